"""The five BASELINE.json configurations as runnable train steps on synthetic inputs of their shape, on one
GPU or 1-D vertex-partitioned over the ranks of a process group.  Used by bench.py (`--workload`) and the tools; the recipes
are the reference's (model shape, drop rates, loss, optimizer), the data is seeded noise — there are no datasets here.

| workload | BASELINE config | model | recipe (reference) |
|---|---|---|---|
| cora     | 1 | GCN 2 x 16                          | src/no-sampling/run.py --model=gcn, Adam, logit loss |
| arxiv    | 2 | GAT 3 layers x 3 heads x 250        | run.py:1011-1013: --labels --loss=loge --linear, RMSprop lr 0.002, dropout .75/.25/.1 |
| reddit   | 3 | GCN 3 x 256                         | run.py --model=gcn --norm=batch, Adam |
| proteins | 4 | edge-feature GAT 6 x 6 heads x 80   | src/ogbn-proteins/gat.py:203-207,320-327: BCE-with-logits over 112 tasks, AdamW lr 0.01, edge drop 0.1 |
| products | 5 | GAT 3 x 4 heads x 120               | src/ogbn-products/gat.py:107-118,238,379-386: loge loss, AdamW lr 0.01, edge drop 0.1 |
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from . import ops, synth
from . import nn as bnn
from . import train as T
from .graph import Graph, preprocess, take_rows, to_bidirected
from .nn import edge_gat

NAMES = ("cora", "arxiv", "reddit", "proteins", "products")

ARXIV_GAT = dict(n_layers=3, n_heads=3, n_hidden=250, norm="batch", dropout=0.75, input_drop=0.25, attn_drop=0.1, edge_drop=0.0,
                 non_interactive_attn=False, use_symmetric_norm=False, linear=True, residual=False)


@dataclass
class Workload:
    name: str
    describe: str                 # goes into the bench line's config.workload
    n_nodes: int
    n_edges: int                  # edges of the graph the sparse kernels sweep (after the reference's preprocessing)
    raw_edges: int
    step: object                  # callable: one full train step (zero_grad, forward, loss, backward, optimizer step)
    model: object
    dominant: tuple               # (kernel family, shape key) of the SpMM the roofline object reports, see bot_amd._C._timed
    dominant_shape: tuple         # (H, D, weighted)
    n_local: int                  # destination rows / edges this rank sweeps (== n_nodes / n_edges on one GPU)
    e_local: int
    dataset: object = None
    graph: object = None


def _loge(x, labels):
    y = F.cross_entropy(x, labels[:, 0], reduction="none")
    return torch.log(T.EPSILON + y) - math.log(T.EPSILON)


def _logit(x, labels):
    return F.cross_entropy(x, labels[:, 0], reduction="none")


def _bce(x, labels):
    return F.binary_cross_entropy_with_logits(x, labels.to(x.dtype), reduction="none").mean(1)


def _edge_dataset(name, device, seed, scale):
    """Inputs of the two edge-GAT scripts.  proteins: the raw graph made bidirected, 8 edge features U(0,1), node features =
    sum of incident edge features (ogbn-proteins/gat.py:58), 112 binary tasks; products: `preprocess`, 100 node features."""
    n, e_raw, f, c = synth.SHAPES[name]
    n, e_raw = max(8, int(n * scale)), max(8, int(e_raw * scale))
    s, d = synth.powerlaw_edges(n, e_raw, synth.BASE_SEED + seed, device=device)
    g = Graph(s, d, n)
    g = to_bidirected(g) if name == "proteins" else preprocess(g)
    g.create_formats_()
    gen = torch.Generator().manual_seed(synth.BASE_SEED + 1000 + seed)
    E = g.number_of_edges()
    if name == "proteins":
        efeat = torch.rand(E, 8, generator=gen).to(device)
        labels = (torch.rand(n, c, generator=gen) < 0.5).to(torch.int64).to(device)
        feat = None
    else:
        efeat = None
        feat = torch.randn(n, f, generator=gen).to(device)
        labels = torch.randint(0, c, (n, 1), generator=gen).to(device)
    perm = torch.randperm(n, generator=gen).to(device)
    a, b = int(0.54 * n), int(0.72 * n)
    ds = synth.Dataset(g, feat, labels, perm[:a], perm[a:b], perm[b:], c, e_raw)
    ds.efeat = efeat
    return ds


MODEL_DIMS = {       # name: (layers, heads, head width, edge-feature GAT)
    "cora": (2, 1, 16, False), "arxiv": (3, 3, 250, False), "reddit": (3, 1, 256, False), "proteins": (6, 6, 80, True), "products": (3, 4, 120, True)}


def hbm_budget(name: str, world: int = 1, scale: float = 1.0) -> dict:
    """A COARSE per-rank estimate (bytes) of what `build` + one step allocate, printed by bench.py before anything is allocated so that a
    first multi-GPU run that cannot fit says so instead of dying in the allocator.  Every rank builds the whole seeded
    dataset on its own device and cuts its block out of it (`build`), so the build term does not shrink with the world size; the step
    term does.  Calibrated on the measured single-GPU peaks (tools/hbm_peak.py, profiles/r05_hbm_peak.txt: 0.18 / 7.1 / 23.8 / 39.4 /
    75.2 GiB for configs 1-5; the estimate lands within +25 % of each; bench.py treats it as a gate that ALL ranks take together and that
    `--ignore-hbm-budget` overrides):
      build  80 B per edge (COO pairs, CSC, CSR, permutations, plans) + node features (+ 32 B per edge of edge features, config 4)
      step   GAT family: 9 B per edge, head and layer (attention weights, their dropped copy / signs) + 7.5 fp32 [rows, H D] tensors per
             wide layer (projection output, gradient operand, pre-BatchNorm state, halves, temporaries); GCN: 150 B per edge (the
             L2-blocked sweep's streams) + the same node term; x 1.3 (the bench process also runs parity / baseline legs: its peaks were 31.6 / 47.2 / 80.3 GiB).  Rows = owned + halo, the halo bounded by all other ranks' rows."""
    n, e_raw, f, c = synth.SHAPES[name]
    n, e_raw = max(8, int(n * scale)), max(8, int(e_raw * scale))
    E = 2 * e_raw + n                                            # symmetrised + self-loops (an upper bound: duplicates merge)
    layers, H, D, edge = MODEL_DIMS[name]
    gcn = name in ("cora", "reddit")
    n_own = -(-n // world)
    n_ext = n if world > 1 else n_own                            # a power-law graph's halo is most of the other ranks' rows
    e_loc = -(-E // world)
    build = E * 80 + n * max(f, 8) * 4 + (E * 32 if name == "proteins" else 0)
    if world > 1:
        build += e_loc * 80 + n_ext * max(f, 8) * 4              # the rank's block beside the whole graph it was cut from
    edge_part = e_loc * 150 if gcn else layers * e_loc * H * 9
    # (the modular edge-GAT stacks keep fewer [rows, H D] temporaries alive than the fused GAT layers: 4.5 against 7.5 tensors per wide layer,
    # recalibrated on profiles/r05_hbm_peak.txt after ADVICE r5: S-products 75.2 GiB measured, 112.5 estimated before, 78 now)
    node_part = max(1, layers - 1) * n_ext * H * D * 4 * (4.5 if edge else 7.5)
    step = int(1.3 * (edge_part + node_part))
    return {"whole_graph_build": int(build), "step": step, "total": int(build) + step + (1 << 28)}      # + 0.25 GiB of fixed costs


def build(name: str, device, *, rank=0, world=1, partitioned=False, seed=0, scale=1.0, norm_adj="rw", partitioner="contiguous",
          group=None, drop=True, capture=False, n_label_iters=0) -> Workload:
    """Dataset + model + optimizer + step of one configuration.  Every rank builds the same (seeded) whole dataset on its own
    device and cuts its block out of it there (bot_amd.dist.build_partition).  `drop=False` zeroes every drop rate (parity
    and CPU tests; the benchmark keeps the reference's rates).  `capture=True`: the step is captured into a hipGraph after 3 eager
    warm-up steps and replayed (bot_amd.train.CapturedTrainStep; the GCN / GAT stacks of configs 1-3, whose step draws no
    host-side seeds per step — the edge-drop mask of configs 4 / 5 does, those stay eager).  `n_label_iters`: label-reuse iterations of the
    workloads that train with labels (arxiv)."""
    k = 1.0 if drop else 0.0
    if name not in NAMES:
        raise ValueError(f"unknown workload {name!r}: {NAMES}")
    dev = torch.device(device)
    if partitioned:
        from . import dist as bdist
    edge = name in ("proteins", "products")
    kw = None                     # keywords of train.train_step (the GCN / GAT stacks)
    ds = _edge_dataset(name, dev, seed, scale) if edge else synth.make_dataset(name, device=dev, seed=seed, scale=scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    torch.manual_seed(seed)
    if name == "arxiv":
        cfg = dict(ARXIV_GAT, use_symmetric_norm=norm_adj == "symm")
        cfg.update(dropout=0.75 * k, input_drop=0.25 * k, attn_drop=0.1 * k)
        model = bnn.GAT(dim_node=ds.feat.shape[1] + C, dim_edge=0, dim_output=C, activation=F.relu, **cfg).to(dev)
        from . import optim as boptim
        opt = boptim.RMSprop(model.parameters(), lr=0.002, capturable=capture)      # torch.optim.RMSprop's update in one launch
        kw = dict(use_labels=True, mask_rate=0.5, loss="loge", n_classes=C)
        if n_label_iters:       # label reuse (run.py:274-279, --n-label-iters); 0 leaves the step's keywords as they were
            kw["n_label_iters"] = int(n_label_iters)
        shape, desc = (3, 250, True), (f"GAT 3 layers x 3 heads x 250, --labels --loss=loge --linear --norm=batch"
                                       f"{' --norm-adj=symm' if norm_adj == 'symm' else ''}, dropout 0.75/0.25/0.1, RMSprop step included")
    elif name in ("cora", "reddit"):
        hid, layers = (16, 2) if name == "cora" else (256, 3)
        model = bnn.GCN(in_feats=ds.feat.shape[1], n_classes=C, n_hidden=hid, n_layers=layers, activation=F.relu,
                        norm="none" if name == "cora" else "batch", norm_adj="symm", dropout=0.5 * k).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.01, capturable=capture, fused=dev.type == "cuda")
        kw = dict(use_labels=False, mask_rate=0.5, loss="logit", n_classes=C)   # run.py:265-267: the mask split also without --labels
        shape, desc = (1, hid, False), f"GCN {layers} layers x {hid}, norm_adj=symm, dropout 0.5, logit loss, Adam step included"
    elif name == "proteins":
        model = edge_gat.ProteinsGAT(node_feats=8, edge_feats=8, n_classes=C, n_layers=6, n_heads=6, n_hidden=80, edge_emb=16,
                                     activation=F.relu, dropout=0.25 * k, input_drop=0.1 * k, attn_drop=0.0, edge_drop=0.1 * k,
                                     allow_zero_in_degree=True).to(dev)
        opt = torch.optim.AdamW(model.parameters(), lr=0.01, weight_decay=0, fused=dev.type == "cuda")
        shape, desc = (6, 80, True), ("edge-feature GAT 6 layers x 6 heads x 80, 8-d edge features, edge_emb 16, dropout 0.25/0.1, "
                                      "edge drop 0.1, BCE-with-logits over 112 tasks, AdamW step included")
    else:
        model = edge_gat.ProductsGAT(node_feats=ds.feat.shape[1], edge_feats=0, n_classes=C, n_layers=3, n_heads=4, n_hidden=120,
                                     edge_emb=0, activation=F.relu, dropout=0.5 * k, input_drop=0.1 * k, attn_drop=0.0, edge_drop=0.1 * k).to(dev)
        opt = torch.optim.AdamW(model.parameters(), lr=0.01, weight_decay=0, fused=dev.type == "cuda")
        shape, desc = (4, 120, True), ("GAT 3 layers x 4 heads x 120, dropout 0.5/0.1, edge drop 0.1, loge loss, AdamW step included")

    if name == "proteins":  # node features = sum of the incident edge features over the WHOLE graph (ogbn-proteins/gat.py:58)
        with torch.no_grad():
            ds.feat = ops.copy_e_sum(g, ds.efeat)
    n_local, e_local = n, E
    if not partitioned:
        if edge:
            g.ndata["feat"] = ds.feat
            if ds.efeat is not None:
                g.edata["feat"] = ds.efeat
            node_loss = _bce if name == "proteins" else _loge
            tr = ds.train_idx

            def step():
                model.train()
                opt.zero_grad()
                pred = model(g)
                loss = node_loss(pred[tr], ds.labels[tr]).mean()
                loss.backward()
                opt.step()
                return loss, pred
        else:
            def step():
                return T.train_step(model, g, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, **kw)
    else:
        part = bdist.partition_dataset(ds, rank, world, dev, group, partitioner=partitioner)
        model = bdist.wrap_model(model, group)
        bdist.seed_rank_streams(seed, rank)
        n_local, e_local = part.n_owned, part.n_edges
        if edge:
            pg = part.graph
            pg.ndata["feat"] = part.feat
            if ds.efeat is not None:
                pg.edata["feat"] = take_rows(ds.efeat, part.edge_ids)
            node_loss = _bce if name == "proteins" else _loge

            def step():
                return bdist.step_generic(lambda: model(pg), part, node_loss, model=model, optimizer=opt, group=group)
        else:
            dkw = {k: v for k, v in kw.items()}

            def step():
                return bdist.train_step(model, part, opt, group=group, **dkw)
        ds.part = part
    captured = False
    if capture and not edge:
        eager, captured = step, True
        step = T.CapturedTrainStep(lambda: eager()[:2], dev)
    H, D, weighted = shape
    describe = (f"S-{name}: power-law graph N={n} E={E} (raw {ds.raw_edges}), F={0 if ds.feat is None else ds.feat.shape[1]}, C={C}; {desc}")
    wl = Workload(name, describe, n, E, ds.raw_edges, step, model, ("spmm", shape), shape, n_local, e_local, ds, g)
    wl.captured = captured
    wl.optimizer = opt
    wl.step_kw = kw
    return wl


SAMPLED = {   # name: (fan-out per layer, batches per epoch over the training nodes) — ogbn-products/gat.py:196-206, ogbn-proteins/gat.py:174-185
    "products": (8, 30), "proteins": (32, 10),
    # the reference trains these three full-batch only (src/no-sampling): their sampled form is this project's choice, products-like —
    # 10 in-edges per layer, 30 batches per epoch (S-cora: 5, its 1 462 training nodes would leave batches of 49 seeds)
    "arxiv": (10, 30), "reddit": (10, 30), "cora": (10, 5)}


@dataclass
class SampledWorkload:
    name: str
    describe: str
    model: object
    optimizer: object
    loader: object                # bot_amd.sampling.NodeDataLoader over the training nodes
    loss: object                  # mean loss of (pred, labels) over a batch's output nodes
    labels: torch.Tensor
    dataset: object
    graph: object
    use_labels: bool = False      # S-arxiv (--labels): the training labels of the input nodes beyond the outputs enter as features
    n_classes: int = 0
    eval_fanouts: object = None   # the evaluation loader's fan-out per layer and seeds per batch (SAMPLED_EVAL); it is built on first use
    eval_batch_size: int = 0
    evaluator: object = None      # bot_amd.metrics.Evaluator of the workload's dataset
    seed: int = 0
    _eval_loader: object = None

    @property
    def eval_loader(self):
        """NodeDataLoader over ALL nodes in node order (ogbn-proteins/gat.py:191-201), built on first use: a workload that never
        evaluates allocates nothing for it."""
        if self._eval_loader is None:
            from .sampling import MultiLayerNeighborSampler, NodeDataLoader
            g = self.graph
            nodes = torch.arange(g.number_of_nodes(), dtype=self.dataset.train_idx.dtype, device=self.dataset.train_idx.device)
            self._eval_loader = NodeDataLoader(g, nodes, MultiLayerNeighborSampler(list(self.eval_fanouts)), batch_size=self.eval_batch_size,
                                               shuffle=False, seed=self.seed + 1)
        return self._eval_loader

    def evaluate(self, evaluator=None, eval_times=1):
        """`minibatch.evaluate_scores` over the evaluation loader: (train_score, val_score, test_score, train_loss, val_loss,
        test_loss, preds) with the workload's loss and, by default, its dataset's `metrics.Evaluator` (one grouped call)."""
        from . import minibatch
        ds = self.dataset
        ev = self.evaluator if evaluator is None else evaluator
        if ev is None:
            raise ValueError(f"S-{self.name} has no OGB metric: pass evaluator=callable(pred, labels)")
        return minibatch.evaluate_scores(self.model, self.eval_loader, self.labels, ds.train_idx, ds.val_idx, ds.test_idx, self.loss, ev,
                                         eval_times=eval_times, use_labels=self.use_labels, n_classes=self.n_classes)

    def inputs(self, blocks):
        """The batch's input features, blocks[0].srcdata["feat"]: gathered from the parent, plus the label columns with `use_labels`
        (minibatch.add_labels, once per batch)."""
        b = blocks[0]
        if self.use_labels and not getattr(b, "_bot_labels_added", False):
            from . import minibatch
            n_out = blocks[-1].number_of_dst_nodes()
            minibatch.add_labels(b, torch.arange(n_out, b.number_of_src_nodes(), device=b.device), self.n_classes)
            b._bot_labels_added = True
        return b.srcdata["feat"]

    def step(self, blocks, output_nodes):
        """One mini-batch train step on sampled blocks (zero_grad, forward, loss, backward, optimizer step); returns the loss."""
        self.model.train()
        self.optimizer.zero_grad()
        self.inputs(blocks)                                   # (the stacks read blocks[0].srcdata["feat"])
        loss = self.loss(self.model(blocks), self.labels[output_nodes])
        loss.backward()
        self.optimizer.step()
        return loss

    def epoch(self):
        """One epoch of `bot_amd.minibatch.train_epoch` over the loader; returns the count-weighted mean loss."""
        from . import minibatch
        return minibatch.train_epoch(self.model, self.loader, self.labels, self.optimizer, self.loss, use_labels=self.use_labels,
                                     n_classes=self.n_classes)


SAMPLED_WEIGHT = "prob"   # the edata column build_sampled(prob=True) samples in proportion to


def sampled_edge_weight(name: str, g, seed=0) -> torch.Tensor:
    """The workload's own per-edge sampling weight, float32 [E] in edge-id order: S-proteins the mean of its 8 edge features (the
    association scores of ogbn-proteins), the others a seeded uniform column on (0, 1]."""
    if name == "proteins":
        return g.edata["feat"].mean(1).contiguous()
    gen = torch.Generator().manual_seed(int(seed) + 0x5EED)
    return (1.0 - torch.rand(g.number_of_edges(), generator=gen)).to(g.device)


SAMPLED_EVAL = {   # name: (evaluation fan-out per layer, seeds per batch given the node count) — ogbn-proteins/gat.py:191-201 (100 in-edges,
    # 65 536 seeds); ogbn-products/gat.py:217-232 (8 in-edges, one thirtieth of the nodes); the others as products
    "proteins": (100, lambda n: 65536), "products": (8, lambda n: -(-n // 30)),
    "arxiv": (10, lambda n: -(-n // 30)), "reddit": (10, lambda n: -(-n // 30)), "cora": (10, lambda n: -(-n // 5))}
OGB_NAMES = {"proteins": "ogbn-proteins", "products": "ogbn-products", "arxiv": "ogbn-arxiv"}


def build_sampled(name: str, device, *, scale=1.0, seed=0, fanouts=None, batch_size=None, drop=True, prob=None, eval_fanouts=None,
                  eval_batch_size=None) -> SampledWorkload:
    """Mini-batch (neighbour-sampled) training: the dataset, model, optimizer and drop rates of `build(name)` (same seeds, same
    BASELINE model definitions), trained on `bot_amd.sampling` blocks with the fan-outs and batch counts of SAMPLED by default
    (products: 8 per layer, ceil(n_train / 30) seeds per batch; proteins: 32 per layer, ceil(n_train / 10); arxiv / reddit: 10 per
    layer, ceil(n_train / 30); cora: 10, ceil(n_train / 5)).  S-arxiv keeps --labels in the sampled form of the products script: the
    training labels of the input nodes beyond the outputs enter as features (ndata["train_labels_onehot"], minibatch.add_labels).
    In-edges are drawn uniformly, or with `prob` in proportion to per-edge weights: an edata key or a tensor, or True for the
    workload's own weights (sampled_edge_weight, stored as edata[SAMPLED_WEIGHT]).
    `eval_fanouts` / `eval_batch_size`: the loader of `SampledWorkload.evaluate()` over all nodes (defaults SAMPLED_EVAL: proteins
    100 per layer and 65 536 seeds per batch, products 8 per layer and ceil(n / 30)); it is built when first used."""
    if name not in SAMPLED:
        raise ValueError(f"sampled training serves {tuple(SAMPLED)}, not {name!r}")
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    wl = build(name, device, seed=seed, scale=scale, drop=drop)
    ds, g = wl.dataset, wl.graph
    fan, parts = SAMPLED[name]
    n_layers = MODEL_DIMS[name][0]
    fanouts = [fan] * n_layers if fanouts is None else list(fanouts)
    n_train = int(ds.train_idx.numel())
    batch_size = -(-n_train // parts) if batch_size is None else int(batch_size)
    if prob is True:
        g.edata[SAMPLED_WEIGHT] = sampled_edge_weight(name, g, seed)
        prob = SAMPLED_WEIGHT
    use_labels = name == "arxiv"
    if name not in ("products", "proteins"):      # the full-batch step hands the features to the model; blocks gather them from ndata
        g.ndata["feat"] = ds.feat
        if use_labels:
            onehot = torch.zeros((g.number_of_nodes(), ds.n_classes), dtype=ds.feat.dtype, device=ds.feat.device)
            onehot[ds.train_idx, ds.labels[ds.train_idx, 0]] = 1.0
            g.ndata["train_labels_onehot"] = onehot
    sampler = MultiLayerNeighborSampler(fanouts, prob=prob)
    loader = NodeDataLoader(g, ds.train_idx, sampler, batch_size=batch_size, shuffle=True, seed=seed)
    node_loss = {"proteins": _bce, "products": _loge, "arxiv": _loge}.get(name, _logit)
    weighted = "" if prob is None else f" (edge-weighted: {prob if isinstance(prob, str) else 'tensor'})"
    describe = (f"S-{name} sampled: fan-outs {fanouts}{weighted}, {batch_size} seeds per batch, {len(loader)} batches per epoch; "
                + wl.describe.split(": ", 1)[1])
    efan, ebatch = SAMPLED_EVAL[name]
    eval_fanouts = [efan] * n_layers if eval_fanouts is None else list(eval_fanouts)
    eval_batch_size = ebatch(g.number_of_nodes()) if eval_batch_size is None else int(eval_batch_size)
    evaluator = None
    if name in OGB_NAMES:
        from .metrics import Evaluator
        evaluator = Evaluator(OGB_NAMES[name])
    return SampledWorkload(name, describe, wl.model, wl.optimizer, loader, lambda x, y: node_loss(x, y).mean(), ds.labels, ds, g,
                           use_labels, ds.n_classes, eval_fanouts, eval_batch_size, evaluator, seed)


SAGE_NAMES = ("cora", "arxiv", "reddit")


def build_sage(name: str, device, *, aggregator="mean", sampled=False, scale=1.0, seed=0, drop=True):
    """GraphSAGE on the dataset and seeds of `build(name)` ("cora", "arxiv", "reddit"): `nn.GraphSAGE` with 3 layers x 256 (cora: 2 x
    16), BatchNorm except on cora, dropout 0.5, one of the aggregators "mean" / "gcn" / "pool"; Adam at 0.01, logit loss, no label
    input.  Full-batch: a `Workload` whose step is `train.train_step`; `sampled=True`: a `SampledWorkload` over neighbour-sampled
    blocks with SAMPLED[name]'s fan-outs and batch counts."""
    if name not in SAGE_NAMES:
        raise ValueError(f"build_sage serves {SAGE_NAMES}, not {name!r}")
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    ds = synth.make_dataset(name, device=dev, seed=seed, scale=scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    torch.manual_seed(seed)
    hid, layers = (16, 2) if name == "cora" else (256, 3)
    model = bnn.GraphSAGE(in_feats=ds.feat.shape[1], n_classes=C, n_hidden=hid, n_layers=layers, activation=F.relu,
                          aggregator_type=aggregator, norm="none" if name == "cora" else "batch", dropout=0.5 * k).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    kw = dict(use_labels=False, mask_rate=0.5, loss="logit", n_classes=C)
    desc = f"GraphSAGE ({aggregator}) {layers} layers x {hid}, dropout 0.5, logit loss, Adam step included"
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}"
    if not sampled:
        def step():
            return T.train_step(model, g, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, **kw)
        family = ("spmm_max", (hid, True)) if aggregator == "pool" else ("spmm", (1, hid, True))
        wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, family, (1, hid, aggregator != "pool"), n, E, ds, g)
        wl.captured, wl.optimizer, wl.step_kw = False, opt, kw
        return wl
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    fan, parts = SAMPLED[name]
    g.ndata["feat"] = ds.feat
    batch_size = -(-int(ds.train_idx.numel()) // parts)
    loader = NodeDataLoader(g, ds.train_idx, MultiLayerNeighborSampler([fan] * layers), batch_size=batch_size, shuffle=True, seed=seed)
    efan, ebatch = SAMPLED_EVAL[name]
    evaluator = None
    if name in OGB_NAMES:
        from .metrics import Evaluator
        evaluator = Evaluator(OGB_NAMES[name])
    describe = f"S-{name} sampled: fan-outs {[fan] * layers}, {batch_size} seeds per batch, {len(loader)} batches per epoch; {head}"
    return SampledWorkload(name, describe, model, opt, loader, lambda x, y: _logit(x, y).mean(), ds.labels, ds, g, False, C,
                           [efan] * layers, ebatch(n), evaluator, seed)


def _build_propagation(who, name, device, scale, seed, make_model, desc):
    """What build_appnp and build_gcn2 share: the dataset and seeds of `build(name)`, Adam at 0.01, logit loss, no label input, a
    full-batch `Workload` whose step is `train.train_step` (not captured: the edge-drop seed would be baked into the launches)."""
    if name not in SAGE_NAMES:
        raise ValueError(f"{who} serves {SAGE_NAMES}, not {name!r}")
    dev = torch.device(device)
    ds = synth.make_dataset(name, device=dev, seed=seed, scale=scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    torch.manual_seed(seed)
    model = make_model(ds.feat.shape[1], C).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    kw = dict(use_labels=False, mask_rate=0.5, loss="logit", n_classes=C)

    def step():
        return T.train_step(model, g, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, **kw)
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}, logit loss, Adam step included"
    wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, ("appnp_step", None), (1, C, False), n, E, ds, g)
    wl.captured, wl.optimizer, wl.step_kw = False, opt, kw
    return wl


def build_appnp(name: str, device, *, scale=1.0, seed=0, drop=True):
    """APPNP on the dataset and seeds of `build(name)` ("cora", "arxiv", "reddit"): `nn.APPNP` with an MLP of 3 x 256 (cora: 2 x 64),
    k = 10, alpha = 0.1, edge dropout 0.5, dropout 0.5; Adam at 0.01, logit loss, no label input.  Full-batch, `train.train_step`."""
    k = 1.0 if drop else 0.0
    hid, layers = (64, 2) if name == "cora" else (256, 3)
    make = lambda fin, C: bnn.APPNP(fin, C, hid, layers, F.relu, k=10, alpha=0.1, edge_drop=0.5 * k, dropout=0.5 * k)
    return _build_propagation("build_appnp", name, device, scale, seed, make, f"APPNP MLP {layers} x {hid}, k=10, alpha=0.1, edge dropout 0.5, dropout 0.5")


def build_gcn2(name: str, device, *, scale=1.0, seed=0, drop=True):
    """GCNII on the dataset and seeds of `build(name)` ("cora", "arxiv", "reddit"): `nn.GCNII` with 16 layers x 256 (cora: 64 x 64),
    alpha = 0.1, lambda = 0.5, dropout 0.5; Adam at 0.01, logit loss, no label input.  Full-batch, `train.train_step`."""
    k = 1.0 if drop else 0.0
    hid, layers = (64, 64) if name == "cora" else (256, 16)
    make = lambda fin, C: bnn.GCNII(fin, C, hid, layers, F.relu, alpha=0.1, lambda_=0.5, dropout=0.5 * k)
    return _build_propagation("build_gcn2", name, device, scale, seed, make, f"GCNII {layers} layers x {hid}, alpha=0.1, lambda=0.5, dropout 0.5")


def build_pna(name: str, device, *, sampled=False, scale=1.0, seed=0, drop=True, num_towers=1):
    """PNA on the dataset and seeds of `build(name)` ("cora", "arxiv", "reddit"): `nn.PNA` with 3 layers x 256 (cora: 2 x 16), the
    mean / max / min / std aggregators times the identity / amplification / attenuation scalers, delta = `nn.pna_delta` of the graph,
    dropout 0.5; Adam at 0.01, logit loss, no label input.  Full-batch: a `Workload` whose step is `train.train_step`; `sampled=True`:
    a `SampledWorkload` over neighbour-sampled blocks with SAMPLED[name]'s fan-outs and batch counts."""
    if name not in SAGE_NAMES:
        raise ValueError(f"build_pna serves {SAGE_NAMES}, not {name!r}")
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    ds = synth.make_dataset(name, device=dev, seed=seed, scale=scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    torch.manual_seed(seed)
    hid, layers = (16, 2) if name == "cora" else (256, 3)
    model = bnn.PNA(in_feats=ds.feat.shape[1], n_classes=C, n_hidden=hid, n_layers=layers, delta=bnn.pna_delta(g), num_towers=num_towers,
                    dropout=0.5 * k).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    kw = dict(use_labels=False, mask_rate=0.5, loss="logit", n_classes=C)
    desc = f"PNA {layers} layers x {hid}, {num_towers} tower(s), 4 aggregators x 3 scalers, dropout 0.5, logit loss, Adam step included"
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}"
    if not sampled:
        def step():
            return T.train_step(model, g, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, **kw)
        wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, ("spmm_pna", (hid, hid // num_towers, 3, 4)), (1, hid, False), n,
                      E, ds, g)
        wl.captured, wl.optimizer, wl.step_kw = False, opt, kw
        return wl
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    fan, parts = SAMPLED[name]
    g.ndata["feat"] = ds.feat
    batch_size = -(-int(ds.train_idx.numel()) // parts)
    loader = NodeDataLoader(g, ds.train_idx, MultiLayerNeighborSampler([fan] * layers), batch_size=batch_size, shuffle=True, seed=seed)
    efan, ebatch = SAMPLED_EVAL[name]
    evaluator = None
    if name in OGB_NAMES:
        from .metrics import Evaluator
        evaluator = Evaluator(OGB_NAMES[name])
    describe = f"S-{name} sampled: fan-outs {[fan] * layers}, {batch_size} seeds per batch, {len(loader)} batches per epoch; {head}"
    return SampledWorkload(name, describe, model, opt, loader, lambda x, y: _logit(x, y).mean(), ds.labels, ds, g, False, C,
                           [efan] * layers, ebatch(n), evaluator, seed)


GATV2_DIMS = {"cora": (2, 8, 8), "arxiv": (3, 3, 250), "reddit": (3, 1, 256)}      # name: (layers, heads, head width)


def build_gatv2(name: str, device, *, sampled=False, scale=1.0, seed=0, drop=True):
    """GATv2 on the dataset and seeds of `build(name)` ("cora", "arxiv", "reddit"): `nn.GATv2` with GATV2_DIMS[name]'s layers x heads x
    head width (arxiv: 3 x 3 x 250, the size of config 2, so the step stands beside the headline GAT step), one output head, BatchNorm
    except on cora, dropout 0.5, attention dropout 0.1; Adam at 0.01, logit loss, no label input.  Full-batch: a `Workload` whose step
    is `train.train_step`; `sampled=True`: a `SampledWorkload` over neighbour-sampled blocks with SAMPLED[name]'s fan-outs and batch
    counts.  The datasets carry self-loops (`build`'s preprocessing), the sampled blocks may not: the layers allow zero in-degree."""
    if name not in GATV2_DIMS:
        raise ValueError(f"build_gatv2 serves {tuple(GATV2_DIMS)}, not {name!r}")
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    ds = synth.make_dataset(name, device=dev, seed=seed, scale=scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    torch.manual_seed(seed)
    layers, heads, hid = GATV2_DIMS[name]
    model = bnn.GATv2(in_feats=ds.feat.shape[1], n_classes=C, n_hidden=hid, n_layers=layers, n_heads=heads, activation=F.relu,
                      norm="none" if name == "cora" else "batch", dropout=0.5 * k, attn_drop=0.1 * k, allow_zero_in_degree=True).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    kw = dict(use_labels=False, mask_rate=0.5, loss="logit", n_classes=C)
    desc = f"GATv2 {layers} layers x {heads} heads x {hid}, dropout 0.5, attention dropout 0.1, logit loss, Adam step included"
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}"
    if not sampled:
        def step():
            return T.train_step(model, g, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, **kw)
        wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, ("gatv2_logits", (heads, hid)), (heads, hid, True), n, E, ds, g)
        wl.captured, wl.optimizer, wl.step_kw = False, opt, kw
        return wl
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    fan, parts = SAMPLED[name]
    g.ndata["feat"] = ds.feat
    batch_size = -(-int(ds.train_idx.numel()) // parts)
    loader = NodeDataLoader(g, ds.train_idx, MultiLayerNeighborSampler([fan] * layers), batch_size=batch_size, shuffle=True, seed=seed)
    efan, ebatch = SAMPLED_EVAL[name]
    evaluator = None
    if name in OGB_NAMES:
        from .metrics import Evaluator
        evaluator = Evaluator(OGB_NAMES[name])
    describe = f"S-{name} sampled: fan-outs {[fan] * layers}, {batch_size} seeds per batch, {len(loader)} batches per epoch; {head}"
    return SampledWorkload(name, describe, model, opt, loader, lambda x, y: _logit(x, y).mean(), ds.labels, ds, g, False, C,
                           [efan] * layers, ebatch(n), evaluator, seed)


GATED_DIMS = {"cora": (2, 64), "arxiv": (3, 256), "reddit": (3, 256)}      # name: (layers, width)


def build_gated(name: str, device, *, sampled=False, normalize=True, scale=1.0, seed=0, drop=True):
    """The residual gated graph ConvNet on the dataset and seeds of `build(name)` ("cora", "arxiv", "reddit"): `nn.ResGatedGCN` with
    GATED_DIMS[name]'s layers x width (arxiv: 3 x 256), GatedGCN's normalised gates unless `normalize=False`, BatchNorm except on cora,
    dropout 0.5; Adam at 0.01, logit loss, no label input.  Full-batch: a `Workload` whose step is `train.train_step`; `sampled=True`: a
    `SampledWorkload` over neighbour-sampled blocks with SAMPLED[name]'s fan-outs and batch counts."""
    if name not in GATED_DIMS:
        raise ValueError(f"build_gated serves {tuple(GATED_DIMS)}, not {name!r}")
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    ds = synth.make_dataset(name, device=dev, seed=seed, scale=scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    torch.manual_seed(seed)
    layers, hid = GATED_DIMS[name]
    model = bnn.ResGatedGCN(in_feats=ds.feat.shape[1], n_classes=C, n_hidden=hid, n_layers=layers, activation=F.relu,
                            norm="none" if name == "cora" else "batch", dropout=0.5 * k, normalize=normalize).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    kw = dict(use_labels=False, mask_rate=0.5, loss="logit", n_classes=C)
    desc = f"ResGatedGCN {layers} layers x {hid}, {'normalised' if normalize else 'plain'} gates, dropout 0.5, logit loss, Adam step included"
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}"
    if not sampled:
        def step():
            return T.train_step(model, g, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, **kw)
        wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, ("spmm_gate", (hid, bool(normalize))), (1, hid, False), n, E, ds, g)
        wl.captured, wl.optimizer, wl.step_kw = False, opt, kw
        return wl
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    fan, parts = SAMPLED[name]
    g.ndata["feat"] = ds.feat
    batch_size = -(-int(ds.train_idx.numel()) // parts)
    loader = NodeDataLoader(g, ds.train_idx, MultiLayerNeighborSampler([fan] * layers), batch_size=batch_size, shuffle=True, seed=seed)
    efan, ebatch = SAMPLED_EVAL[name]
    evaluator = None
    if name in OGB_NAMES:
        from .metrics import Evaluator
        evaluator = Evaluator(OGB_NAMES[name])
    describe = f"S-{name} sampled: fan-outs {[fan] * layers}, {batch_size} seeds per batch, {len(loader)} batches per epoch; {head}"
    return SampledWorkload(name, describe, model, opt, loader, lambda x, y: _logit(x, y).mean(), ds.labels, ds, g, False, C,
                           [efan] * layers, ebatch(n), evaluator, seed)


GATEDGCN_NAMES = ("arxiv", "proteins")
GATEDGCN_DIMS = (3, 128)            # layers, width
GATEDGCN_EDGE_FEATS = 8
GATEDGCN_EDGE_MATRICES = 6          # [E, width] float32 matrices a training layer keeps for its backward: C's output e_hat (also the
                                    # BatchNorm's input), the BatchNorm + ReLU output, the residual sum, the dropout output (the next
                                    # layer's C input) and its mask's worth, the upstream gradient in flight
GATEDGCN_HBM_BYTES = 288e9          # one MI355X


def _gatedgcn_parts(name, device, scale, seed, drop, full_batch):
    """Dataset, model, optimiser, per-node loss and description that the two GatedGCN recipes share."""
    if name not in GATEDGCN_NAMES:
        raise ValueError(f"the GatedGCN recipes serve {GATEDGCN_NAMES}, not {name!r}")
    layers, hid = GATEDGCN_DIMS
    if full_batch:
        _, e_raw, _, _ = synth.SHAPES[name]
        need = 2.2 * e_raw * scale * hid * 4 * GATEDGCN_EDGE_MATRICES * layers      # (bidirected, or preprocessed: about 2.2 edges per raw edge)
        if need > 0.8 * GATEDGCN_HBM_BYTES:
            raise ValueError(f'build_gatedgcn("{name}", scale={scale}): the edge stream of a full-batch step needs about {need / 1e9:.0f} GB '
                             f"({GATEDGCN_EDGE_MATRICES} [E, {hid}] float32 matrices per layer), more than one device holds; train on subgraphs: "
                             f'workloads.build_gatedgcn_clustered("{name}", ...)')
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    if name == "proteins":
        ds = _edge_dataset(name, dev, seed, scale)
        g = ds.graph
        with torch.no_grad():       # node features = sum of the incident edge features over the WHOLE graph, as in build("proteins")
            ds.feat = ops.copy_e_sum(g, ds.efeat)
        node_loss = _bce
    else:
        ds = synth.make_dataset(name, device=dev, seed=seed, scale=scale)
        g = ds.graph
        gen = torch.Generator().manual_seed(synth.BASE_SEED + 2000 + seed)
        ds.efeat = torch.randn(g.number_of_edges(), GATEDGCN_EDGE_FEATS, generator=gen).to(dev)
        node_loss = _logit
    g.ndata["feat"], g.edata["feat"] = ds.feat, ds.efeat
    torch.manual_seed(seed)
    model = bnn.GatedGCN(in_feats=ds.feat.shape[1], edge_in_feats=int(ds.efeat.shape[1]), n_classes=ds.n_classes, n_hidden=hid,
                         n_layers=layers, dropout=0.5 * k).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    n, E = g.number_of_nodes(), g.number_of_edges()
    desc = (f"GatedGCN (edge stream, {int(ds.efeat.shape[1])} raw edge features) {layers} layers x {hid}, BatchNorm, residual, dropout 0.5, "
            f"{'BCE-with-logits over %d tasks' % ds.n_classes if name == 'proteins' else 'logit loss'}, Adam step included")
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={ds.n_classes}; {desc}"
    return ds, g, model, opt, node_loss, head


def build_gatedgcn(name: str, device, *, scale=1.0, seed=0, drop=True):
    """GatedGCN with an edge stream, full-batch: `nn.GatedGCN` with 3 layers x 128 (the benchmark's depth is 4 x 70 on its small graphs;
    128 is the width the sweeps are measured at), BatchNorm, residual, dropout 0.5, Adam at 0.01.  "proteins": the dataset of
    `build("proteins")` with its 8 raw edge features and BCE over the tasks; "arxiv": the dataset of `build("arxiv")` with seeded normal
    [E, 8] edge features and the logit loss.  A plain `Workload` whose step runs forward, loss, backward and the optimiser step.
    Memory: [E, 128] is the model's state - at S-arxiv one [E, 128] float32 matrix is 1.28 GB and a training step keeps about
    GATEDGCN_EDGE_MATRICES of them per layer.  "proteins" at scale 1.0 (79 M edges: 40 GB per matrix) does not fit full-batch and is
    refused with a pointer to `build_gatedgcn_clustered`."""
    ds, g, model, opt, node_loss, head = _gatedgcn_parts(name, device, scale, seed, drop, True)
    tr = ds.train_idx

    def step():
        model.train()
        opt.zero_grad()
        pred = model(g, ds.feat)
        loss = node_loss(pred[tr], ds.labels[tr]).mean()
        loss.backward()
        opt.step()
        return loss, pred
    hid = GATEDGCN_DIMS[1]
    n, E = g.number_of_nodes(), g.number_of_edges()
    wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, ("spmm_gate_edge", (hid, True, True)), (1, hid, False), n, E, ds, g)
    wl.captured, wl.optimizer, wl.step_kw = False, opt, None
    return wl


def build_gatedgcn_clustered(name: str, device, *, scale=1.0, seed=0, n_parts=None, parts_per_batch=1, method="community", drop=True):
    """The model, dataset and optimiser of `build_gatedgcn(name)` on induced-subgraph (Cluster-GCN) batches: a `SubgraphWorkload` with
    `node_loss` and a `ClusterLoader` over CLUSTERED[name] parts (or `n_parts`).  A batch gathers its node and edge features from the
    parent's frames, and its edge ids are its CSC positions, so the edge stream needs no permutation.  This is how the model fits
    S-proteins."""
    from . import minibatch
    from .sampling import ClusterLoader, cluster_assignment
    ds, g, model, opt, node_loss, head = _gatedgcn_parts(name, device, scale, seed, drop, False)
    roles = minibatch.node_roles(g.number_of_nodes(), ds.train_idx, ds.val_idx, ds.test_idx)
    n_parts = min(CLUSTERED[name] if n_parts is None else int(n_parts), g.number_of_nodes())
    parts = cluster_assignment(g, n_parts, method, seed)
    loader = ClusterLoader(g, parts, parts_per_batch=parts_per_batch, shuffle=True, seed=seed)
    describe = f"S-{name} clustered: {n_parts} parts ({method}), {parts_per_batch} per batch, {len(loader)} batches per epoch; {head}"
    return SubgraphWorkload(name, describe, model, opt, loader, ds.labels, roles, ds, g, None, node_loss, parts)


def build_rgcn(name: str, device, *, num_rels=8, regularizer="basis", num_bases=4, sampled=False, scale=1.0, seed=0, drop=True):
    """The relational GCN on the dataset and seeds of `build(name)` ("cora", "arxiv", "reddit"): `nn.RGCN` with GATED_DIMS[name]'s
    layers x width, `num_rels` relations drawn per edge as seeded uniform integers (g.edata["etype"]) with the entity-classification norm
    `nn.rel_norm` (g.edata["norm"]), the basis regulariser with `num_bases` bases (num_bases=None or regularizer=None: one weight per
    relation), BatchNorm except on cora, dropout 0.5; Adam at 0.01, logit loss, no label input.  Labels and relations are noise: the
    recipe measures a step and claims no accuracy.  Full-batch: a `Workload` whose step is `train.train_step`; `sampled=True`: a
    `SampledWorkload` over neighbour-sampled blocks with SAMPLED[name]'s fan-outs and batch counts (a block's frames gather the
    relations and the norm from the parent)."""
    if name not in GATED_DIMS:
        raise ValueError(f"build_rgcn serves {tuple(GATED_DIMS)}, not {name!r}")
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    ds = synth.make_dataset(name, device=dev, seed=seed, scale=scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    gen = torch.Generator().manual_seed(seed + 1)
    g.edata["etype"] = torch.randint(0, num_rels, (E,), generator=gen, dtype=torch.int32).to(dev)
    g.edata["norm"] = bnn.rel_norm(g, "etype", num_rels)
    torch.manual_seed(seed)
    layers, hid = GATED_DIMS[name]
    model = bnn.RGCN(in_feats=ds.feat.shape[1], n_classes=C, n_hidden=hid, n_layers=layers, num_rels=num_rels, activation=F.relu,
                     regularizer=regularizer, num_bases=num_bases, norm="none" if name == "cora" else "batch", dropout=0.5 * k).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    kw = dict(use_labels=False, mask_rate=0.5, loss="logit", n_classes=C)
    B = model.convs[0].num_bases
    desc = (f"RGCN {layers} layers x {hid}, {num_rels} relations, {f'{B} bases' if B < num_rels else 'one weight per relation'}, "
            "dropout 0.5, logit loss, Adam step included")
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}"
    if not sampled:
        def step():
            return T.train_step(model, g, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, **kw)
        wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, ("spmm_rel_expand", (hid, num_rels, B if B < num_rels else 0)),
                      (1, hid, False), n, E, ds, g)
        wl.captured, wl.optimizer, wl.step_kw = False, opt, kw
        return wl
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    fan, parts = SAMPLED[name]
    g.ndata["feat"] = ds.feat
    batch_size = -(-int(ds.train_idx.numel()) // parts)
    loader = NodeDataLoader(g, ds.train_idx, MultiLayerNeighborSampler([fan] * layers), batch_size=batch_size, shuffle=True, seed=seed)
    efan, ebatch = SAMPLED_EVAL[name]
    evaluator = None
    if name in OGB_NAMES:
        from .metrics import Evaluator
        evaluator = Evaluator(OGB_NAMES[name])
    describe = f"S-{name} sampled: fan-outs {[fan] * layers}, {batch_size} seeds per batch, {len(loader)} batches per epoch; {head}"
    return SampledWorkload(name, describe, model, opt, loader, lambda x, y: _logit(x, y).mean(), ds.labels, ds, g, False, C,
                           [efan] * layers, ebatch(n), evaluator, seed)


UNIMP_DIMS = {"cora": (2, 8, 8), "arxiv": (3, 3, 250), "reddit": (3, 1, 256)}      # name: (layers, heads, head width)


def build_unimp(name: str, device, *, sampled=False, scale=1.0, seed=0, drop=True, use_labels=True):
    """UniMP (Shi et al., arXiv:2009.03509) on the dataset and seeds of `build(name)` ("cora", "arxiv", "reddit"): `nn.UniMP` with
    UNIMP_DIMS[name]'s layers x heads x head width (arxiv: 3 x 3 x 250, the size of config 2), the gated residual, BatchNorm except on
    cora, dropout 0.5, attention dropout 0.1; Adam at 0.01, logit loss.  `use_labels`: the paper's masked label prediction - the
    training labels enter as input columns under a random mask (rate 0.5), wired as `build("arxiv")` does for --labels
    (`train.train_step(use_labels=True)`; sampled: ndata["train_labels_onehot"], minibatch.add_labels).  Full-batch: a `Workload` whose
    step is `train.train_step`; `sampled=True`: a `SampledWorkload` over neighbour-sampled blocks with SAMPLED[name]'s fan-outs and
    batch counts."""
    if name not in UNIMP_DIMS:
        raise ValueError(f"build_unimp serves {tuple(UNIMP_DIMS)}, not {name!r}")
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    ds = synth.make_dataset(name, device=dev, seed=seed, scale=scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    torch.manual_seed(seed)
    layers, heads, hid = UNIMP_DIMS[name]
    model = bnn.UniMP(in_feats=ds.feat.shape[1] + (C if use_labels else 0), n_classes=C, n_hidden=hid, n_layers=layers, n_heads=heads,
                      activation=F.relu, norm="none" if name == "cora" else "batch", dropout=0.5 * k, attn_drop=0.1 * k).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    kw = dict(use_labels=bool(use_labels), mask_rate=0.5, loss="logit", n_classes=C)
    desc = (f"UniMP {layers} layers x {heads} heads x {hid}{', masked label input' if use_labels else ''}, dropout 0.5, attention dropout "
            f"0.1, logit loss, Adam step included")
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}"
    if not sampled:
        def step():
            return T.train_step(model, g, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, **kw)
        wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, ("dot_attn", (heads, hid, False)), (heads, hid, True), n, E, ds, g)
        wl.captured, wl.optimizer, wl.step_kw = False, opt, kw
        return wl
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    fan, parts = SAMPLED[name]
    g.ndata["feat"] = ds.feat
    if use_labels:
        onehot = torch.zeros((n, C), dtype=ds.feat.dtype, device=ds.feat.device)
        onehot[ds.train_idx, ds.labels[ds.train_idx, 0]] = 1.0
        g.ndata["train_labels_onehot"] = onehot
    batch_size = -(-int(ds.train_idx.numel()) // parts)
    loader = NodeDataLoader(g, ds.train_idx, MultiLayerNeighborSampler([fan] * layers), batch_size=batch_size, shuffle=True, seed=seed)
    efan, ebatch = SAMPLED_EVAL[name]
    evaluator = None
    if name in OGB_NAMES:
        from .metrics import Evaluator
        evaluator = Evaluator(OGB_NAMES[name])
    describe = f"S-{name} sampled: fan-outs {[fan] * layers}, {batch_size} seeds per batch, {len(loader)} batches per epoch; {head}"
    return SampledWorkload(name, describe, model, opt, loader, lambda x, y: _logit(x, y).mean(), ds.labels, ds, g, bool(use_labels), C,
                           [efan] * layers, ebatch(n), evaluator, seed)


GEN_NAMES = ("cora", "arxiv", "reddit")


def build_gen(name: str, device, *, sampled=False, scale=1.0, seed=0, drop=True, learn_beta=True):
    """DeeperGCN on the dataset and seeds of `build(name)` ("cora", "arxiv", "reddit"): `nn.DeeperGCN` with 3 GENConv layers x 256 (cora:
    2 x 16), softmax aggregation with beta = 1.0 (learned with `learn_beta`), dropout 0.5; Adam at 0.01, logit loss, no label input.
    Full-batch: a `Workload` whose step is `train.train_step`; `sampled=True`: a `SampledWorkload` over neighbour-sampled blocks with
    SAMPLED[name]'s fan-outs and batch counts."""
    if name not in GEN_NAMES:
        raise ValueError(f"build_gen serves {GEN_NAMES}, not {name!r}")
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    ds = synth.make_dataset(name, device=dev, seed=seed, scale=scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    torch.manual_seed(seed)
    hid, layers = (16, 2) if name == "cora" else (256, 3)
    model = bnn.DeeperGCN(in_feats=ds.feat.shape[1], n_classes=C, n_hidden=hid, n_layers=layers, dropout=0.5 * k, beta=1.0,
                          learn_beta=learn_beta).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    kw = dict(use_labels=False, mask_rate=0.5, loss="logit", n_classes=C)
    desc = (f"DeeperGCN (softmax, beta 1.0{' learned' if learn_beta else ''}) {layers} layers x {hid}, dropout 0.5, logit loss, "
            f"Adam step included")
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}"
    if not sampled:
        def step():
            return T.train_step(model, g, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, **kw)
        family = ("spmm_softmax", (hid, True, bool(learn_beta)))       # `_C._timed`'s key of the layers' forward sweep
        wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, family, (1, hid, False), n, E, ds, g)
        wl.captured, wl.optimizer, wl.step_kw = False, opt, kw
        return wl
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    fan, parts = SAMPLED[name]
    g.ndata["feat"] = ds.feat
    batch_size = -(-int(ds.train_idx.numel()) // parts)
    loader = NodeDataLoader(g, ds.train_idx, MultiLayerNeighborSampler([fan] * layers), batch_size=batch_size, shuffle=True, seed=seed)
    efan, ebatch = SAMPLED_EVAL[name]
    evaluator = None
    if name in OGB_NAMES:
        from .metrics import Evaluator
        evaluator = Evaluator(OGB_NAMES[name])
    describe = f"S-{name} sampled: fan-outs {[fan] * layers}, {batch_size} seeds per batch, {len(loader)} batches per epoch; {head}"
    return SampledWorkload(name, describe, model, opt, loader, lambda x, y: _logit(x, y).mean(), ds.labels, ds, g, False, C,
                           [efan] * layers, ebatch(n), evaluator, seed)


GEN_EDGE_NAMES = ("proteins",)


def build_gen_edge(name: str, device, *, sampled=False, scale=1.0, seed=0, drop=True, learn_beta=True):
    """DeeperGCN with edge features on the dataset, seeds, node features and loss of `build("proteins")` (8 raw edge features, node
    features = the sum of the incident edge features, BCE-with-logits over 112 tasks): `nn.DeeperGCN(edge_dim=8)` with 3 GENConv
    layers x 256 - the width at which the other recipes measure the sweeps; the paper's own 64 is a row of tools/bench_gen_edge.py -
    softmax aggregation with beta = 1.0 (learned with `learn_beta`), dropout 0.5, Adam at 0.01.  Every layer projects the raw edge
    features inside its sweep (`ops.u_add_e_softmax`).  Full-batch: a `Workload`; `sampled=True`: a `SampledWorkload` over
    neighbour-sampled blocks with SAMPLED["proteins"]'s fan-outs and batch counts and the ROC-AUC evaluator."""
    if name not in GEN_EDGE_NAMES:
        raise ValueError(f"build_gen_edge serves {GEN_EDGE_NAMES}, not {name!r}")
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    ds = _edge_dataset(name, dev, seed, scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    K = int(ds.efeat.shape[1])
    with torch.no_grad():       # node features = sum of the incident edge features over the WHOLE graph, as in build("proteins")
        ds.feat = ops.copy_e_sum(g, ds.efeat)
    g.ndata["feat"], g.edata["feat"] = ds.feat, ds.efeat
    torch.manual_seed(seed)
    hid, layers = 256, 3
    model = bnn.DeeperGCN(in_feats=ds.feat.shape[1], n_classes=C, n_hidden=hid, n_layers=layers, dropout=0.5 * k, beta=1.0,
                          learn_beta=learn_beta, edge_dim=K).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    desc = (f"DeeperGCN (softmax, beta 1.0{' learned' if learn_beta else ''}, edge_dim {K}) {layers} layers x {hid}, dropout 0.5, "
            f"BCE-with-logits over {C} tasks, Adam step included")
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}"
    if not sampled:
        tr = ds.train_idx

        def step():
            model.train()
            opt.zero_grad()
            pred = model(g, ds.feat)
            loss = _bce(pred[tr], ds.labels[tr]).mean()
            loss.backward()
            opt.step()
            return loss, pred
        family = ("spmm_softmax_edge", (hid, K, True, bool(learn_beta)))     # `_C._timed`'s key of the layers' forward sweep
        wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, family, (1, hid, False), n, E, ds, g)
        wl.captured, wl.optimizer, wl.step_kw = False, opt, None
        return wl
    from .metrics import Evaluator
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    fan, parts = SAMPLED[name]
    batch_size = -(-int(ds.train_idx.numel()) // parts)
    loader = NodeDataLoader(g, ds.train_idx, MultiLayerNeighborSampler([fan] * layers), batch_size=batch_size, shuffle=True, seed=seed)
    efan, ebatch = SAMPLED_EVAL[name]
    describe = f"S-{name} sampled: fan-outs {[fan] * layers}, {batch_size} seeds per batch, {len(loader)} batches per epoch; {head}"
    return SampledWorkload(name, describe, model, opt, loader, lambda x, y: _bce(x, y).mean(), ds.labels, ds, g, False, C,
                           [efan] * layers, ebatch(n), Evaluator(OGB_NAMES[name]), seed)


PNA_EDGE_NAMES = ("proteins",)


def build_pna_edge(name: str, device, *, sampled=False, scale=1.0, seed=0, drop=True, num_towers=1):
    """PNA with edge features on the data of `build_gen_edge("proteins")` - its dataset, seeds, node features (the sum of the incident
    edge features) and BCE-with-logits loss over 112 tasks: `nn.EdgePNA(edge_dim=8)` with 3 layers x 256, the mean / max / min / std
    aggregators times the identity / amplification / attenuation scalers of `build_pna`, delta = `nn.pna_delta` of the graph, dropout
    0.5; Adam at 0.01.  Every layer projects the 8 raw edge features inside its sweep (`ops.pna_aggregate_edge`).  Full-batch: a
    `Workload`; `sampled=True`: a `SampledWorkload` over neighbour-sampled blocks with SAMPLED["proteins"]'s fan-outs and batch counts
    and the ROC-AUC evaluator."""
    if name not in PNA_EDGE_NAMES:
        raise ValueError(f"build_pna_edge serves {PNA_EDGE_NAMES}, not {name!r}")
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    ds = _edge_dataset(name, dev, seed, scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    K = int(ds.efeat.shape[1])
    with torch.no_grad():       # node features = sum of the incident edge features over the WHOLE graph, as in build("proteins")
        ds.feat = ops.copy_e_sum(g, ds.efeat)
    g.ndata["feat"], g.edata["feat"] = ds.feat, ds.efeat
    torch.manual_seed(seed)
    hid, layers = 256, 3
    model = bnn.EdgePNA(in_feats=ds.feat.shape[1], n_classes=C, n_hidden=hid, n_layers=layers, edge_dim=K, delta=bnn.pna_delta(g),
                        num_towers=num_towers, dropout=0.5 * k).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    desc = (f"PNA (edge_dim {K}) {layers} layers x {hid}, {num_towers} tower(s), 4 aggregators x 3 scalers, dropout 0.5, "
            f"BCE-with-logits over {C} tasks, Adam step included")
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}"
    if not sampled:
        tr = ds.train_idx

        def step():
            model.train()
            opt.zero_grad()
            pred = model(g, ds.feat)
            loss = _bce(pred[tr], ds.labels[tr]).mean()
            loss.backward()
            opt.step()
            return loss, pred
        family = ("spmm_pna_edge", (hid, hid // num_towers, K, 3, 4))        # `_C._timed`'s key of the layers' forward sweep
        wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, family, (1, hid, False), n, E, ds, g)
        wl.captured, wl.optimizer, wl.step_kw = False, opt, None
        return wl
    from .metrics import Evaluator
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    fan, parts = SAMPLED[name]
    batch_size = -(-int(ds.train_idx.numel()) // parts)
    loader = NodeDataLoader(g, ds.train_idx, MultiLayerNeighborSampler([fan] * layers), batch_size=batch_size, shuffle=True, seed=seed)
    efan, ebatch = SAMPLED_EVAL[name]
    describe = f"S-{name} sampled: fan-outs {[fan] * layers}, {batch_size} seeds per batch, {len(loader)} batches per epoch; {head}"
    return SampledWorkload(name, describe, model, opt, loader, lambda x, y: _bce(x, y).mean(), ds.labels, ds, g, False, C,
                           [efan] * layers, ebatch(n), Evaluator(OGB_NAMES[name]), seed)


UNIMP_EDGE_NAMES = ("proteins",)
UNIMP_EDGE_DIMS = (3, 4, 64)      # layers, heads, head width: H * D = 256, the width build_gen_edge measures at


def build_unimp_edge(name: str, device, *, sampled=False, scale=1.0, seed=0, drop=True):
    """UniMP with edge features on the data of `build_gen_edge("proteins")` - its dataset, seeds, node features (the sum of the incident
    edge features), BCE-with-logits loss over 112 tasks, step and sampled loader: `nn.EdgeUniMP(edge_dim=8)` with 3 layers x 4 heads x
    64, the gated residual, BatchNorm, dropout 0.5, attention dropout 0.1; Adam at 0.01, no label input.  Every layer reads the 8 raw
    edge features inside its attention sweep (`ops.dot_attention_edge`).  Full-batch: a `Workload`; `sampled=True`: a
    `SampledWorkload` over neighbour-sampled blocks with SAMPLED["proteins"]'s fan-outs and batch counts and the ROC-AUC evaluator."""
    if name not in UNIMP_EDGE_NAMES:
        raise ValueError(f"build_unimp_edge serves {UNIMP_EDGE_NAMES}, not {name!r}")
    k = 1.0 if drop else 0.0
    dev = torch.device(device)
    ds = _edge_dataset(name, dev, seed, scale)
    g = ds.graph
    n, E, C = g.number_of_nodes(), g.number_of_edges(), ds.n_classes
    K = int(ds.efeat.shape[1])
    with torch.no_grad():       # node features = sum of the incident edge features over the WHOLE graph, as in build("proteins")
        ds.feat = ops.copy_e_sum(g, ds.efeat)
    g.ndata["feat"], g.edata["feat"] = ds.feat, ds.efeat
    torch.manual_seed(seed)
    layers, heads, hid = UNIMP_EDGE_DIMS
    model = bnn.EdgeUniMP(in_feats=ds.feat.shape[1], n_classes=C, n_hidden=hid, n_layers=layers, n_heads=heads, activation=F.relu, norm="batch",
                          dropout=0.5 * k, attn_drop=0.1 * k, edge_dim=K).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=dev.type == "cuda")
    desc = (f"UniMP (edge_dim {K}) {layers} layers x {heads} heads x {hid}, dropout 0.5, attention dropout 0.1, BCE-with-logits over {C} "
            f"tasks, Adam step included")
    head = f"power-law graph N={n} E={E} (raw {ds.raw_edges}), F={ds.feat.shape[1]}, C={C}; {desc}"
    if not sampled:
        tr = ds.train_idx

        def step():
            model.train()
            opt.zero_grad()
            pred = model(g, ds.feat)
            loss = _bce(pred[tr], ds.labels[tr]).mean()
            loss.backward()
            opt.step()
            return loss, pred
        family = ("dot_attn_edge", (heads, hid, K))     # `_C._timed`'s key of the layers' forward sweep
        wl = Workload(name, f"S-{name}: {head}", n, E, ds.raw_edges, step, model, family, (heads, hid, True), n, E, ds, g)
        wl.captured, wl.optimizer, wl.step_kw = False, opt, None
        return wl
    from .metrics import Evaluator
    from .sampling import MultiLayerNeighborSampler, NodeDataLoader
    fan, parts = SAMPLED[name]
    batch_size = -(-int(ds.train_idx.numel()) // parts)
    loader = NodeDataLoader(g, ds.train_idx, MultiLayerNeighborSampler([fan] * layers), batch_size=batch_size, shuffle=True, seed=seed)
    efan, ebatch = SAMPLED_EVAL[name]
    describe = f"S-{name} sampled: fan-outs {[fan] * layers}, {batch_size} seeds per batch, {len(loader)} batches per epoch; {head}"
    return SampledWorkload(name, describe, model, opt, loader, lambda x, y: _bce(x, y).mean(), ds.labels, ds, g, False, C,
                           [efan] * layers, ebatch(n), Evaluator(OGB_NAMES[name]), seed)


CLUSTERED = {name: batches for name, (_, batches) in SAMPLED.items()}    # default part counts: the batch counts of SAMPLED


@dataclass
class SubgraphWorkload:
    """Training on induced-subgraph batches: `build_clustered` (parts set) and `build_saint` (loss_weight and presample_s set)."""
    name: str
    describe: str
    model: object
    optimizer: object
    loader: object                # bot_amd.sampling.ClusterLoader / SAINTLoader over the whole graph
    labels: torch.Tensor
    roles: torch.Tensor           # minibatch.node_roles of the dataset's split
    dataset: object
    graph: object
    step_kw: dict = None          # GCN / GAT stacks: the keywords of train.train_step
    node_loss: object = None      # edge-feature stacks: per-node loss of (pred, labels)
    parts: torch.Tensor = None    # clustered: int32 [N], the part of every node
    loss_weight: torch.Tensor = None   # SAINT: float32 [N], original node order (sampling.saint_loss_weights); None = unweighted
    presample_s: float = 0.0      # SAINT: wall time of the one-off pre-sampling
    edge_weight: str = None       # SAINT with aggregator_norm: the edata key of sampling.saint_norms' edge_norm; None = unit weights

    def _edge_kw(self):
        return {} if self.edge_weight is None else {"edge_weight": self.edge_weight}

    def step(self, sub):
        """One train step on a batch (bot_amd.minibatch.subgraph_step): (loss, pred, training nodes) or None."""
        from . import minibatch
        return minibatch.subgraph_step(self.model, sub, self.optimizer, self.labels, self.roles, node_loss=self.node_loss,
                                       step_kw=self.step_kw, loss_weight=self.loss_weight, **self._edge_kw())

    def epoch(self):
        """One epoch of `bot_amd.minibatch.train_epoch_subgraphs`: (training-count-weighted mean loss, skipped batches)."""
        from . import minibatch
        ds = self.dataset
        return minibatch.train_epoch_subgraphs(self.model, self.loader, self.optimizer, self.labels, ds.train_idx, val_idx=ds.val_idx,
                                               test_idx=ds.test_idx, node_loss=self.node_loss, step_kw=self.step_kw,
                                               loss_weight=self.loss_weight, **self._edge_kw())


def _subgraph_base(name: str, device, kind: str, **build_kw) -> SubgraphWorkload:
    """What `build_clustered` and `build_saint` compute alike: `build(name)` as a SubgraphWorkload that still lacks its loader,
    with `describe` holding the model's part only (the builder puts its own in front)."""
    if name not in CLUSTERED:
        raise ValueError(f"{kind} training serves {tuple(CLUSTERED)}, not {name!r}")
    from . import minibatch
    wl = build(name, device, **build_kw)
    ds, g = wl.dataset, wl.graph
    if wl.step_kw is not None:        # the full-batch step hands the features to the model; a batch gathers them from ndata
        g.ndata["feat"] = ds.feat
    node_loss = None if wl.step_kw is not None else (_bce if name == "proteins" else _loge)
    roles = minibatch.node_roles(g.number_of_nodes(), ds.train_idx, ds.val_idx, ds.test_idx)
    return SubgraphWorkload(name, wl.describe.split(": ", 1)[1], wl.model, wl.optimizer, None, ds.labels, roles, ds, g, wl.step_kw, node_loss)


def build_clustered(name: str, device, *, scale=1.0, seed=0, n_parts=None, parts_per_batch=1, method="community", drop=True,
                    n_label_iters=0) -> SubgraphWorkload:
    """Induced-subgraph (Cluster-GCN) training: the dataset, model, optimizer and drop rates of `build(name)` (same seeds, same
    BASELINE model definitions); the vertices are cut into `n_parts` parts (default CLUSTERED: 30 / 30 / 5 / 30 / 10 for arxiv /
    reddit / cora / products / proteins) by `sampling.cluster_assignment(method)`, and every step runs the full-batch step on the
    subgraph that `parts_per_batch` parts induce, with the training nodes that fall inside it.  S-proteins' node features stay the
    whole graph's sums of incident edge features."""
    from .sampling import ClusterLoader, cluster_assignment
    wl = _subgraph_base(name, device, "clustered", seed=seed, scale=scale, drop=drop, n_label_iters=n_label_iters)
    g = wl.graph
    n_parts = min(CLUSTERED[name] if n_parts is None else int(n_parts), g.number_of_nodes())
    wl.parts = cluster_assignment(g, n_parts, method, seed)
    wl.loader = ClusterLoader(g, wl.parts, parts_per_batch=parts_per_batch, shuffle=True, seed=seed)
    wl.describe = (f"S-{name} clustered: {n_parts} parts ({method}), {parts_per_batch} per batch, {len(wl.loader)} batches per epoch; "
                   + wl.describe)
    return wl


SAINT_NORM = "saint_norm"   # the edata column build_saint(aggregator_norm=True) stores the per-edge normalisation in
SAINT_GCN = ("reddit", "cora")   # the GCN recipes: the stacks that take the aggregator normalisation
SAINT_COVERAGE = 50    # GraphSAINT's default sample_coverage: pre-sampled visits per node, on average


def saint_defaults(name: str, n_nodes: int, *, mode="walk", length=2, n_batches=None, n_presample=None):
    """(budget, n_batches, n_presample) of `build_saint`, all derived: n_batches = CLUSTERED[name]; walk mode (n_roots, length) with
    n_roots = ceil(N / (n_batches (length + 1))), so a batch holds at most the node count of one cluster part; node mode n_draws =
    ceil(N / n_batches); n_presample = 50 n_batches (GraphSAINT's sample_coverage of 50 visits per node on average)."""
    if name not in CLUSTERED:
        raise ValueError(f"SAINT training serves {tuple(CLUSTERED)}, not {name!r}")
    n_batches = CLUSTERED[name] if n_batches is None else int(n_batches)
    length = int(length)
    if n_batches < 1 or length < 0:
        raise ValueError(f"n_batches={n_batches} length={length}")
    if mode == "walk":
        budget = (-(-int(n_nodes) // (n_batches * (length + 1))), length)
    elif mode == "node":
        budget = -(-int(n_nodes) // n_batches)
    else:
        raise ValueError(f"build_saint takes mode 'walk' or 'node', not {mode!r}")
    return budget, n_batches, SAINT_COVERAGE * n_batches if n_presample is None else int(n_presample)


def build_saint(name: str, device, *, scale=1.0, seed=0, mode="walk", length=2, n_batches=None, n_presample=None, drop=True,
                n_label_iters=0, aggregator_norm=False) -> SubgraphWorkload:
    """GraphSAINT training: the dataset, model, optimizer and drop rates of `build(name)` (same seeds, same BASELINE model
    definitions); every step runs the full-batch step on the subgraph induced by the nodes that `sampling.SAINTSampler(mode)`
    reaches (budgets: `saint_defaults`; length = 2 is the GraphSAINT paper's random-walk setting), with the training nodes that fall
    inside it, their loss weighted by `sampling.saint_loss_weights` (pre-sampled once, here).  The walks start at any node, as
    the cluster parts cover every node.  `aggregator_norm` (the GCN recipes "reddit" and "cora" only; a GAT stack learns its edge
    weights): the same pre-sampling also yields GraphSAINT's per-edge aggregator normalisation (`sampling.saint_norms`), stored as
    g.edata[SAINT_NORM]; every batch hands its rows to the stack's layers as `edge_weight` (`wl.edge_weight` names the column)."""
    import time
    from .sampling import SAINTLoader, SAINTSampler, saint_loss_weights, saint_norms
    if aggregator_norm and name not in SAINT_GCN:
        raise ValueError(f"aggregator_norm is for the GCN recipes {SAINT_GCN}, not {name!r}: a GAT stack learns its edge weights")
    wl = _subgraph_base(name, device, "SAINT", seed=seed, scale=scale, drop=drop, n_label_iters=n_label_iters)
    g = wl.graph
    budget, n_batches, n_presample = saint_defaults(name, g.number_of_nodes(), mode=mode, length=length, n_batches=n_batches,
                                                    n_presample=n_presample)
    sampler = SAINTSampler(mode, budget)
    t0 = time.perf_counter()
    if aggregator_norm:
        wl.loss_weight, g.edata[SAINT_NORM] = saint_norms(g, sampler, n_presample, seed)
        wl.edge_weight = SAINT_NORM
    else:
        wl.loss_weight = saint_loss_weights(g, sampler, n_presample, seed)
    if wl.loss_weight.is_cuda:
        torch.cuda.synchronize(wl.loss_weight.device)
    wl.presample_s = time.perf_counter() - t0
    wl.loader = SAINTLoader(g, sampler, n_batches, seed=seed)
    form = "loss and aggregator normalisation" if aggregator_norm else "loss normalisation only"
    wl.describe = (f"S-{name} GraphSAINT ({mode}): budget {budget}, {n_batches} batches per epoch, {n_presample} pre-sampled sets, {form}; "
                   + wl.describe)
    return wl
