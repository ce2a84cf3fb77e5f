"""GraphSAINT's node sets restated in numpy (the contracts of bot_saint_walk_i32 / bot_saint_nodes_*_i32, include/bot_gnn.h, and of
`sampling.saint_loss_weights`), shared by tests/test_saint_host.py (where the restatement is itself checked: it walks along edges,
its draws have the stated distributions, and it stands in for the kernels on CPU graphs) and tests/test_saint_gpu.py (which holds
the kernels to it bit for bit)."""
import numpy as np
import torch

from tests.test_sampling_host import philox4x32_10

M64 = (1 << 64) - 1


def draws(seed, walks, step, ranges):
    """umulhi64(x, r) per walk: x = the first 64 bits of Philox4x32-10(seed, walk << 32 | step), word 0 the high half; r < 2^32."""
    walks = np.asarray(walks, dtype=np.uint64)
    m = np.broadcast_to(np.asarray(ranges, dtype=np.uint64), walks.shape)
    assert np.all(m < np.uint64(1 << 32))
    r = philox4x32_10(int(seed) & M64, (walks << np.uint64(32)) | np.uint64(step)).astype(np.uint64)
    hi, lo = r[:, 0], r[:, 1]
    return ((hi * m + ((lo * m) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)     # < 2^64 for r < 2^32: no overflow


def walk_reference(indptr, indices, nids, n_roots, length, root_mode, seed):
    """trace int32 [n_roots, length + 1]: walk i starts at nids[draw] (None: the draw itself; root_mode 1: indices[draw over the
    edges]) and steps to a uniformly drawn in-neighbour (CSC row), staying where a node has none."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n_rows, nnz = len(indptr) - 1, len(indices)
    walks = np.arange(n_roots, dtype=np.int64)
    trace = np.zeros((n_roots, length + 1), dtype=np.int64)
    if n_roots == 0:
        return trace.astype(np.int32)
    if root_mode == 1:
        assert nids is None and nnz > 0
        v = indices[draws(seed, walks, 0, nnz)]
    elif nids is None:
        v = draws(seed, walks, 0, n_rows)
    else:
        nids = np.asarray(nids, dtype=np.int64)
        v = nids[draws(seed, walks, 0, len(nids))]
    trace[:, 0] = v
    for t in range(1, length + 1):
        base, deg = indptr[v], indptr[v + 1] - indptr[v]
        move = deg > 0
        d = draws(seed, walks, t, np.maximum(deg, 1))
        v = np.where(move, indices[np.where(move, base + d, 0)], v)
        trace[:, t] = v
    return trace.astype(np.int32)


def node_set_reference(trace):
    """The distinct entries of the trace, ascending: int32 [n]."""
    return np.unique(np.asarray(trace).reshape(-1)).astype(np.int32)


def sampler_nodes_reference(g, sampler, seed):
    """What `SAINTSampler.sample_nodes(g, seed)` must return (numpy int32)."""
    c = g.csc
    nids = None if sampler.nids is None else sampler.nids.cpu().numpy()
    return node_set_reference(walk_reference(c.indptr.cpu().numpy(), c.indices.cpu().numpy(), nids, sampler.n_roots, sampler.length,
                                             sampler.root_mode, seed))


def presample_seeds(n_presample, seed):
    """The seeds `saint_loss_weights` draws: from its own generator, as MultiLayerNeighborSampler.sample_blocks draws a layer's."""
    gen = torch.Generator().manual_seed(int(seed))
    return [int(torch.randint(-2 ** 63, 2 ** 63 - 1, (), dtype=torch.int64, generator=gen)) for _ in range(n_presample)]


def loss_weights_reference(g, sampler, n_presample, seed=0):
    """(lw float32 [N] in ORIGINAL node order, the pre-sampled sets as ORIGINAL ids, C int64 [N] in original order)."""
    n = g.number_of_nodes()
    perm = np.arange(n) if g.node_perm is None else g.node_perm.cpu().numpy()
    count = np.zeros(n, dtype=np.int64)
    sets = []
    for s in presample_seeds(n_presample, seed):
        nodes = perm[sampler_nodes_reference(g, sampler, s).astype(np.int64)]
        count[nodes] += 1
        sets.append(nodes)
    lw = (np.float32(n_presample) / np.maximum(count, 1).astype(np.float32)).astype(np.float32)
    return lw, sets, count


# ---- CPU stand-ins for the bot_amd._C wrappers (tests/test_saint_host.py installs them)
def saint_walk_standin(csc, nids, n_roots, length, root_mode, seed):
    trace = walk_reference(csc.indptr.cpu().numpy(), csc.indices.cpu().numpy(), None if nids is None else nids.cpu().numpy(), int(n_roots),
                           int(length), int(root_mode), seed)
    return torch.from_numpy(trace).to(csc.indptr.device)


def saint_nodes_standin(trace, node_map):
    ids = trace.cpu().numpy()
    if ids.size and (ids.min() < 0 or ids.max() >= int(node_map.numel())):
        raise ValueError("saint_nodes: entries of the trace lie outside the graph")
    return torch.from_numpy(node_set_reference(ids)).to(trace.device)


def weighted_loss_formula(pred, labels, wn, lw, kind, eps):
    """The weighted loss written out (float64 torch tensors; autograd-able in pred): over the nodes with wn > 0,
    sum lw y / sum lw with ce = logsumexp(x) - x[label]; logit: y = ce, loge: log(eps + ce) - log eps, savage: (1 - exp(-ce))^2."""
    import math
    on = torch.nonzero(wn > 0).squeeze(1)
    x = pred[on]
    lab = labels[on, 0].long()
    ce = torch.logsumexp(x, dim=1) - x[torch.arange(len(on)), lab]
    y = {"logit": ce, "loge": torch.log(eps + ce) - math.log(eps), "savage": (1 - torch.exp(-ce)) ** 2}[kind]
    w = lw[on].to(pred.dtype)
    return (w * y).sum() / w.sum()
