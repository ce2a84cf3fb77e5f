"""Gated aggregation (bot_amd.ops.gated_sum / nn.ResGatedGraphConv / nn.ResGatedGCN, csrc/spmm_gate.hip) measured on one GPU.

  op-arxiv / op-products   `ops.gated_sum` forward and forward + backward (all three gradients), plain and normalised, the kernel form
            against the tensor form (`ops.gated_sum_positions`: gathers to [E, F], sigmoid, segment sums), on S-arxiv at F = 256 and on
            S-products at --products-scale and F = 128 (small enough that the tensor form's [E, F] tensors fit).  The two forms alternate
            in ONE process: --rounds rounds, each the median of --calls calls after --warmup warm-up calls, every call ended by a device
            synchronise; the spread of a form is its largest minus its smallest round.  Peak allocated bytes of both forms beside the
            times, and `kernel_wins_beyond_tensor_spread`: the rule `ops.gate_default_impl` is set by.  Then the three sweeps alone
            (`_C.spmm_gate`, `_C.spmm_gate_bwd_dst`, `_C.spmm_gate_bwd_src`, q and v as the two blocks of one [n, 2F] matrix) beside the
            sum sweep (`_C.spmm` on g.csc / g.csr) at width 2F, each with its byte model (csrc/spmm_gate.hip) and the rate that model
            gives: a gate sweep whose rate falls short of the sum sweep's is limited by its arithmetic (one exponential and two true
            divisions per gathered element), not by the gather.
  step-arxiv     one full-batch train step of `workloads.build_gated("arxiv")`, both forms.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_gated.py [--steps op-arxiv op-products step-arxiv]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = "cuda:0"
EPS = 1e-6


def _sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def _median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(calls):
        t0 = _sync()
        fn()
        times.append(_sync() - t0)
    return 1e3 * statistics.median(times)


def _alternate(forms, a):
    """{name: {"rounds_ms", "median_ms", "spread_ms"}} of forms {name: callable}, alternating round by round."""
    rounds = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():
            rounds[k].append(round(_median_ms(fn, a.calls, a.warmup), 4))
    return {k: {"rounds_ms": v, "median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)} for k, v in rounds.items()}


def _graph(name, scale, a):
    """The workload's graph (the same seeded edges and preprocessing as bot_amd.workloads) without its feature matrix."""
    import bot_amd
    from bot_amd import synth
    n, e_raw, _, _ = synth.SHAPES[name]
    n, e_raw = max(8, int(n * scale)), max(8, int(e_raw * scale))
    s, d = synth.powerlaw_edges(n, e_raw, synth.BASE_SEED + a.seed, device=DEV)
    g = bot_amd.preprocess(bot_amd.Graph(s, d, n))
    _ = g.csr
    return g


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def child_op(name, F, scale, a):
    from bot_amd import _C, ops
    g = _graph(name, scale, a)
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(a.seed + 5)
    k = torch.randn(n, F, generator=gen).to(DEV)
    qv = torch.randn(n, 2 * F, generator=gen).to(DEV)          # the merged projection: q and v are its two column blocks
    q, v = qv[:, :F], qv[:, F:]
    dout = torch.randn(n, F, generator=gen).to(DEV)
    b = torch.randn(n, F, generator=gen).to(DEV)
    out = {"step": a.child, "graph": name, "scale": scale, "n_nodes": n, "n_edges": E, "F": F, "rounds": a.rounds, "calls": a.calls,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    o, den, dk, dqv = (torch.empty(n, w, device=DEV) for w in (F, F, F, 2 * F))
    forms = {"gate_fwd": lambda: _C.spmm_gate(g.csc, k, q, v, out=o),
             "gate_fwd_norm": lambda: _C.spmm_gate(g.csc, k, q, v, True, EPS, out=o, den=den),
             "gate_bwd_dst": lambda: _C.spmm_gate_bwd_dst(g.csc, k, q, v, dout, out=dk),
             "gate_bwd_dst_norm": lambda: _C.spmm_gate_bwd_dst(g.csc, k, q, v, dout, b, out=dk),
             "gate_bwd_src": lambda: _C.spmm_gate_bwd_src(g.csr, k, q, v, dout, out_dq=dqv[:, :F], out_dv=dqv[:, F:]),
             "gate_bwd_src_norm": lambda: _C.spmm_gate_bwd_src(g.csr, k, q, v, dout, b, out_dq=dqv[:, :F], out_dv=dqv[:, F:]),
             "sum_csc_2F": lambda: _C.spmm(g.csc, qv.view(n, 1, 2 * F)), "sum_csr_2F": lambda: _C.spmm(g.csr, qv.view(n, 1, 2 * F))}
    model = {"gate_fwd": 4 * (E * (1 + 2 * F) + 2 * n * F), "gate_fwd_norm": 4 * (E * (1 + 2 * F) + 3 * n * F),
             "gate_bwd_dst": 4 * (E * (1 + 2 * F) + 3 * n * F), "gate_bwd_dst_norm": 4 * (E * (1 + 2 * F) + 4 * n * F),
             "gate_bwd_src": 4 * (E * (1 + 2 * F) + 4 * n * F), "gate_bwd_src_norm": 4 * (E * (1 + 3 * F) + 4 * n * F),
             "sum_csc_2F": 4 * (E * (1 + 2 * F) + 2 * n * F), "sum_csr_2F": 4 * (E * (1 + 2 * F) + 2 * n * F)}
    sweeps = _alternate(forms, a)
    for key, val in sweeps.items():
        val["byte_model"] = model[key]
        val["model_gb_per_s"] = round(model[key] / (val["median_ms"] * 1e-3) / 1e9, 1)
    out["sweeps"] = sweeps
    for key in forms:
        if key.startswith("gate"):
            ref = "sum_csr_2F" if "src" in key else "sum_csc_2F"
            out[f"{key}_rate_over_sum_sweep"] = round(sweeps[key]["model_gb_per_s"] / sweeps[ref]["model_gb_per_s"], 4)
    del forms
    leaves = [t.clone().requires_grad_() for t in (k, q, v)]
    for normalize in (False, True):
        tag = "normalised" if normalize else "plain"

        def fwd(impl):
            with torch.no_grad():
                return ops.gated_sum(g, k, q, v, normalize=normalize, eps=EPS, impl=impl)

        def both(impl):
            for t in leaves:
                t.grad = None
            ops.gated_sum(g, *leaves, normalize=normalize, eps=EPS, impl=impl).backward(dout)
        diff = float((fwd("kernel") - fwd("tensor")).abs().max())
        if not diff <= 1e-3:
            sys.exit(f"the two forms differ by {diff}")
        r = {"max_abs_diff_between_forms": diff}
        r["forward"] = _alternate({i: (lambda i=i: fwd(i)) for i in ("kernel", "tensor")}, a)
        r["forward_backward"] = _alternate({i: (lambda i=i: both(i)) for i in ("kernel", "tensor")}, a)
        r["peak_bytes_forward_backward"] = {i: _peak(lambda i=i: both(i)) for i in ("kernel", "tensor")}
        wins = True
        for key in ("forward", "forward_backward"):
            x = r[key]
            x["kernel_faster_by_ms"] = round(x["tensor"]["median_ms"] - x["kernel"]["median_ms"], 4)
            wins = wins and x["kernel_faster_by_ms"] > x["tensor"]["spread_ms"]
        r["kernel_wins_beyond_tensor_spread"] = wins
        out[tag] = r
    out["kernel_wins_beyond_tensor_spread"] = out["plain"]["kernel_wins_beyond_tensor_spread"] and out["normalised"]["kernel_wins_beyond_tensor_spread"]
    return out


def child_step(a):
    from bot_amd import ops, workloads
    out = {"step": "step-arxiv", "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    wl = workloads.build_gated("arxiv", DEV, scale=a.scale, seed=a.seed)
    out["n_nodes"], out["n_edges"], out["describe"] = wl.n_nodes, wl.n_edges, wl.describe
    old = ops.gate_default_impl

    def step_as(impl):
        def run():
            ops.gate_default_impl = impl
            try:
                wl.step()
            finally:
                ops.gate_default_impl = old
        return run
    forms = {i: step_as(i) for i in ("kernel", "tensor")}
    out["step"] = "step-arxiv"
    out["forms"] = _alternate(forms, a)
    out["peak_bytes"] = {i: _peak(fn) for i, fn in forms.items()}
    return out


CHILDREN = {
    "op-arxiv": lambda a: child_op("arxiv", 256, a.scale, a),
    "op-products": lambda a: child_op("products", 128, a.products_scale, a),
    "step-arxiv": child_step,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=["op-arxiv", "op-products", "step-arxiv"], choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0, help="of S-arxiv")
    ap.add_argument("--products-scale", type=float, default=0.1, help="of S-products where the tensor form runs too")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_gated.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_gated.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [line for line in out.stdout.splitlines() if line.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
