"""Label reuse on the fused glue in the partitioned train step (bot_amd.dist.forward_backward, n_label_iters > 0), world size 2 over gloo
on CPU: kernels emulated (tests/_oracle_backend.py plus the stand-in for the one new wrapper, tests/test_label_reuse_host.py); the
collectives, the partitioning, SyncBatchNorm under no_grad and the control flow are the product's."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_reuse(rank, world, port, partitioner, tmp):
    """bdist.forward_backward(n_label_iters=1) on the new path against the single-process TENSOR-OP form (tolerances of
    tests/test_dist_gloo.py::_worker_extras' label-reuse case)."""
    import types
    import torch.distributed as dist
    import torch.nn.functional as F
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        from tests import _oracle_backend, test_label_reuse_host as H
        _oracle_backend.install_direct()
        import bot_amd
        from bot_amd.nn import fused
        fused.FORCE = True
        from bot_amd import dist as bdist, synth
        from bot_amd import nn as bnn
        from bot_amd import train as T
        from oracle import ref_ops as R
        n, C, fin = 1500, 5, 9
        cs, cd = synth.community_edges(n, 9000, 3, n_blocks=6, p_in=0.9)
        s, d = R.preprocess_edges(cs, cd, n)
        gen = torch.Generator().manual_seed(7)
        feat = torch.randn(n, fin, generator=gen)
        labels = torch.randint(0, C, (n, 1), generator=gen)
        perm = torch.randperm(n, generator=gen)
        tr, va, te = perm[: n // 2], perm[n // 2: 3 * n // 4], perm[3 * n // 4: n - 40]      # 40 nodes in none of the sets
        mask_full = torch.rand(n, generator=gen) < 0.5

        def make():
            torch.manual_seed(3)
            return bnn.GAT(dim_node=fin + C, dim_edge=0, dim_output=C, n_hidden=16, n_layers=3, n_heads=3, activation=F.relu,
                           norm="batch", linear=True)

        g = bot_amd.Graph(s, d, n)
        ref = make().train()
        # the single-process tensor-op form: CPU tensors without the test switch take it (the stand-in is installed only afterwards)
        c0 = H.CALLS[0]
        loss_ref, pred_ref, _ = T.forward_backward(ref, g, feat, labels, tr, va, te, use_labels=True, n_label_iters=1, loss="loge",
                                                   n_classes=C, mask=mask_full[tr])
        H.install_standin()
        ds = types.SimpleNamespace(graph=g, feat=feat, labels=labels, train_idx=tr, val_idx=va, test_idx=te)
        part = bdist.partition_dataset(ds, rank, world, "cpu", partitioner=partitioner)
        ids = part.node_ids if part.node_ids is not None else torch.arange(part.lo, part.hi)
        model = bdist.wrap_model(make().train())
        own_tr = ids[part.train_idx]
        T.DEBUG_KEEP_PREDS, T.DEBUG_PREDS[:] = True, []
        loss, pred = bdist.forward_backward(model, part, use_labels=True, n_label_iters=1, loss="loge", n_classes=C, mask=mask_full[own_tr])
        assert H.CALLS[0] - c0 == 1, H.CALLS                                           # only the partitioned step took the new path, once
        assert len(T.DEBUG_PREDS) == 1 and not T.DEBUG_PREDS[0].requires_grad
        member = T._reuse_members(part.feat.shape[0], part.train_idx, part.val_idx, part.test_idx)
        left_out = torch.isin(ids, perm[n - 40:])
        assert member is not None and torch.equal(member == 0, left_out)
        assert abs(loss.item() - loss_ref.item()) < 1e-5, (loss.item(), loss_ref.item())
        np.testing.assert_allclose(pred.detach().numpy(), pred_ref.detach()[ids].numpy(), rtol=1e-4, atol=2e-5)
        for (k, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
            np.testing.assert_allclose(p.grad.numpy(), q.grad.numpy(), rtol=2e-4, atol=2e-5 * max(1.0, q.grad.abs().max().item()), err_msg=k)
        for (k, b), (_, c) in zip(model.named_buffers(), ref.named_buffers()):
            np.testing.assert_allclose(b.numpy(), c.numpy(), rtol=1e-4, atol=1e-5, err_msg=k)      # running statistics, 2 batches tracked
            if k.endswith("num_batches_tracked"):
                assert int(b) == 2, k
        open(os.path.join(tmp, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("partitioner,world", [("contiguous", 2)])
def test_partitioned_label_reuse_on_the_fused_glue(partitioner, world, tmp_path):
    mp.spawn(_worker_reuse, args=(world, _free_port(), partitioner, str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))
