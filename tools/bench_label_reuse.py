"""Label reuse (n_label_iters > 0, run.py:274-279) on the fused train step against the tensor-op form of the same step, on one GPU.

S-arxiv (bot_amd.workloads.build("arxiv")) at --scale, the reference's drop rates, RMSprop's update inside the timed window.  For every
n_label_iters the two forms - the fused glue (bot_amd.train.FUSED_STEP = True) and the tensor-op form (False: what label reuse ran on before
the fused path existed) - are timed in the SAME process on the same model, alternating, --rounds times: --warmup untimed steps, then
--steps steps between two device events, with the peak of torch's allocated bytes over that window.  One JSON line per configuration,
form and round goes to --out, and one "summary" line per configuration: the mean ms per step of each form, the spread (largest minus
smallest round) of each, and whether the fused form is within / below the tensor-op form's own spread.

    python tools/bench_label_reuse.py [--iters 0 1 2] [--scale 1.0] [--rounds 3] [--warmup 5] [--steps 100] [--out profiles/bench_label_reuse.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def window(wl, warmup, steps):
    """ms per step over `steps` steps between two device events, and the peak allocated bytes of the window."""
    for _ in range(warmup):
        wl.step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss, _ = wl.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, int(torch.cuda.max_memory_allocated()), float(loss)


def run(k, a, emit):
    from bot_amd import _C, train as T, workloads
    torch.manual_seed(a.seed)
    wl = workloads.build("arxiv", torch.device("cuda:0"), seed=a.seed, scale=a.scale, n_label_iters=k)
    res = {"fused": [], "tensor_op": []}
    for rnd in range(a.rounds):
        for form in ("fused", "tensor_op"):
            T.FUSED_STEP = form == "fused"
            calls = _C.REUSE_CALLS
            try:
                ms, peak, loss = window(wl, a.warmup, a.steps)
            finally:
                T.FUSED_STEP = True
            took = (_C.REUSE_CALLS - calls) // (a.warmup + a.steps)
            assert took == (k if form == "fused" else 0), (form, k, took)         # the form that was timed is the form that was asked for
            res[form].append((ms, peak))
            emit({"n_label_iters": k, "form": form, "round": rnd, "ms_per_step": round(ms, 4), "peak_allocated_bytes": peak, "warmup": a.warmup,
                  "steps": a.steps, "scale": a.scale, "last_loss": loss, "nodes": wl.n_nodes, "edges": wl.n_edges,
                  "device": torch.cuda.get_device_name(0)})
    out = {"n_label_iters": k, "summary": True, "scale": a.scale, "rounds": a.rounds, "steps": a.steps}
    for form, rows in res.items():
        ms = [r[0] for r in rows]
        out[form] = {"mean_ms": round(sum(ms) / len(ms), 4), "spread_ms": round(max(ms) - min(ms), 4), "peak_allocated_bytes": max(r[1] for r in rows)}
    diff = out["fused"]["mean_ms"] - out["tensor_op"]["mean_ms"]
    out["fused_minus_tensor_op_ms"] = round(diff, 4)
    out["not_slower"] = diff <= out["tensor_op"]["spread_ms"]                       # not above by more than the tensor-op form's own spread
    out["faster_beyond_spread"] = -diff > out["tensor_op"]["spread_ms"]
    out["peak_not_higher"] = out["fused"]["peak_allocated_bytes"] <= out["tensor_op"]["peak_allocated_bytes"]
    emit(out)
    del wl
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", nargs="+", type=int, default=[0, 1, 2])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_label_reuse.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_label_reuse.py measures on an MI355X: no GPU here")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for k in a.iters:
            run(k, a, emit)


if __name__ == "__main__":
    main()
