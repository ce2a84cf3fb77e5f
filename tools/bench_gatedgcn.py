"""GatedGCN with an edge stream (bot_amd.ops.gated_edge_sum / nn.GatedGCNConv / nn.GatedGCN, csrc/spmm_gate_edge.hip) measured on one GPU.

  op-arxiv-128 / op-arxiv-256 / op-products-128
            `ops.gated_edge_sum(order="csc")`, normalised, forward (no_grad, e returned) and forward + backward (all four gradients,
            an upstream gradient on both outputs), the kernel form against the tensor form (`ops.gated_edge_positions`), on S-arxiv
            at F = 128 and 256 and on S-products at --products-scale and F = 128.  The two forms alternate in ONE process: --rounds
            rounds, each the median of --calls calls after --warmup warm-up calls, every call ended by a device synchronise; the spread
            of a form is its largest minus its smallest round.  Peak allocated bytes of both forms beside the times, and
            `kernel_wins_beyond_tensor_spread`: the rule `ops.gate_edge_default_impl` is set by.  Then every sweep alone
            (`_C.spmm_gate_edge` with and without e, `_C.spmm_gate_edge_bwd` with and without de, `_C.spmm_gate_edge_bwd_src`; q and v
            as the two blocks of one [n, 2F] matrix) beside its byte model (csrc/spmm_gate_edge.hip) and beside the `gated_sum` sweeps
            (csrc/spmm_gate.hip) at the same F, and the two CSC sweeps once more with non-temporal accesses to their streamed rows
            (`stream_nt`): the A/B of `_C.GATE_EDGE_STREAM_NT`.
  step-arxiv   one full-batch train step of `workloads.build_gatedgcn("arxiv")`, both forms, with peak allocated bytes.
  trace        one `rocprofv3 --kernel-trace --stats` run of a child that calls every sweep once on S-arxiv at F = 128 (a run of its own,
            no counters); the sweeps' rows of the kernel statistics go to bench_gatedgcn_kernel_stats.csv beside --out.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_gatedgcn.py [--steps op-arxiv-128 op-arxiv-256 op-products-128 step-arxiv trace]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_gen import _kernel_stats  # noqa: E402

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


def _operands(g, F, a):
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(a.seed + 5)
    r = lambda rows, w: torch.randn(rows, w, generator=gen).to(DEV)
    return dict(k=r(n, F), qv=r(n, 2 * F), c=r(E, F), dout=r(n, F), b=r(n, F), de=r(E, F))


def _sweeps(g, F, x):
    """({name: callable}, {name: byte model}) of every sweep alone, the `gated_sum` sweeps at the same F beside them."""
    from bot_amd import _C
    n, E = g.number_of_nodes(), g.number_of_edges()
    k, qv, c, dout, b, de = (x[i] for i in ("k", "qv", "c", "dout", "b", "de"))
    q, v = qv[:, :F], qv[:, F:]                                  # the merged projection: q and v are its two column blocks
    o, den, dk, dqv = (torch.empty(n, w, device=DEV) for w in (F, F, F, 2 * F))
    e, ds = torch.empty(E, F, device=DEV), torch.empty(E, F, device=DEV)
    _C.spmm_gate_edge(g.csc, k, q, v, c, True, EPS, out=o, den=den, e=e)
    _C.spmm_gate_edge_bwd(g.csc, v, e, dout, b, de, out_ds=ds, out_dk=dk)
    pos = g.csr2csc
    forms, model = {}, {}
    for nt in (False, True):
        tag = "_nt" if nt else ""
        forms["edge_fwd" + tag] = lambda nt=nt: _C.spmm_gate_edge(g.csc, k, q, v, c, True, EPS, out=o, den=den, e=e, stream_nt=nt)
        forms["edge_fwd_no_e" + tag] = lambda nt=nt: _C.spmm_gate_edge(g.csc, k, q, v, c, True, EPS, out=o, den=den, want_e=False, stream_nt=nt)
        forms["edge_bwd_csc" + tag] = lambda nt=nt: _C.spmm_gate_edge_bwd(g.csc, v, e, dout, b, de, out_ds=ds, out_dk=dk, stream_nt=nt)
        forms["edge_bwd_csc_no_de" + tag] = lambda nt=nt: _C.spmm_gate_edge_bwd(g.csc, v, e, dout, b, None, out_ds=ds, out_dk=dk, stream_nt=nt)
        model["edge_fwd" + tag] = 4 * (E * (1 + 2 * F + 2 * F) + 3 * n * F)
        model["edge_fwd_no_e" + tag] = 4 * (E * (1 + 2 * F + F) + 3 * n * F)
        model["edge_bwd_csc" + tag] = 4 * (E * (1 + 4 * F) + 4 * n * F)
        model["edge_bwd_csc_no_de" + tag] = 4 * (E * (1 + 3 * F) + 4 * n * F)
    forms["edge_bwd_csr"] = lambda: _C.spmm_gate_edge_bwd_src(g.csr, pos, e, ds, dout, out_dq=dqv[:, :F], out_dv=dqv[:, F:])
    model["edge_bwd_csr"] = 4 * (E * (2 + 3 * F) + 3 * n * F)
    forms["gate_fwd_norm"] = lambda: _C.spmm_gate(g.csc, k, q, v, True, EPS, out=o, den=den)
    forms["gate_bwd_dst_norm"] = lambda: _C.spmm_gate_bwd_dst(g.csc, k, q, v, dout, b, out=dk)
    forms["gate_bwd_src_norm"] = lambda: _C.spmm_gate_bwd_src(g.csr, k, q, v, dout, b, out_dq=dqv[:, :F], out_dv=dqv[:, F:])
    model["gate_fwd_norm"] = 4 * (E * (1 + 2 * F) + 3 * n * F)
    model["gate_bwd_dst_norm"] = 4 * (E * (1 + 2 * F) + 4 * n * F)
    model["gate_bwd_src_norm"] = 4 * (E * (1 + 3 * F) + 4 * n * F)
    return forms, model


def child_op(name, F, scale, a):
    from bot_amd import ops
    g = _graph(name, scale, a)
    n, E = g.number_of_nodes(), g.number_of_edges()
    x = _operands(g, F, a)
    out = {"step": a.child, "graph": name, "scale": scale, "n_nodes": n, "n_edges": E, "F": F, "rounds": a.rounds, "calls": a.calls,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "edge_matrix_bytes": 4 * E * F}
    forms, model = _sweeps(g, F, x)
    sweeps = _alternate(forms, a)
    for key, val in sweeps.items():
        val["byte_model"] = model[key]
        val["model_gb_per_s"] = round(model[key] / (val["median_ms"] * 1e-3) / 1e9, 1)
    out["sweeps"] = sweeps
    out["stream_nt"] = {}
    for key in ("edge_fwd", "edge_fwd_no_e", "edge_bwd_csc", "edge_bwd_csc_no_de"):
        plain, nt = sweeps[key], sweeps[key + "_nt"]
        gain = round(plain["median_ms"] - nt["median_ms"], 4)
        out["stream_nt"][key] = {"nt_faster_by_ms": gain, "beyond_both_spreads": gain > max(plain["spread_ms"], nt["spread_ms"])}
    del forms
    k, qv, c, dout, de = (x[i] for i in ("k", "qv", "c", "dout", "de"))
    q, v = qv[:, :F], qv[:, F:]
    leaves = [t.clone().requires_grad_() for t in (k, q, v, c)]

    def fwd(impl):
        with torch.no_grad():
            return ops.gated_edge_sum(g, k, q, v, c, normalize=True, eps=EPS, order="csc", impl=impl)

    def both(impl):
        for t in leaves:
            t.grad = None
        o, e = ops.gated_edge_sum(g, *leaves, normalize=True, eps=EPS, order="csc", impl=impl)
        torch.autograd.backward([o, e], [dout, de])
    (ok, ek), (ot, et) = fwd("kernel"), fwd("tensor")
    diff = max(float((ok - ot).abs().max()), float((ek - et).abs().max()))
    del ok, ek, ot, et
    if not diff <= 1e-3:
        sys.exit(f"the two forms differ by {diff}")
    r = {"max_abs_diff_between_forms": diff}
    r["forward"] = _alternate({i: (lambda i=i: fwd(i)) for i in ("kernel", "tensor")}, a)
    r["forward_backward"] = _alternate({i: (lambda i=i: both(i)) for i in ("kernel", "tensor")}, a)
    r["peak_bytes_forward_backward"] = {i: _peak(lambda i=i: both(i)) for i in ("kernel", "tensor")}
    wins = True
    for key in ("forward", "forward_backward"):
        y = r[key]
        y["kernel_faster_by_ms"] = round(y["tensor"]["median_ms"] - y["kernel"]["median_ms"], 4)
        wins = wins and y["kernel_faster_by_ms"] > y["tensor"]["spread_ms"]
    r["kernel_wins_beyond_tensor_spread"] = wins
    out["normalised"] = r
    out["kernel_wins_beyond_tensor_spread"] = wins
    return out


def child_step(a):
    from bot_amd import ops, workloads
    out = {"step": "step-arxiv", "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    wl = workloads.build_gatedgcn("arxiv", DEV, scale=a.scale, seed=a.seed)
    out["n_nodes"], out["n_edges"], out["describe"] = wl.n_nodes, wl.n_edges, wl.describe
    old = ops.gate_edge_default_impl

    def step_as(impl):
        def run():
            ops.gate_edge_default_impl = impl
            try:
                wl.step()
            finally:
                ops.gate_edge_default_impl = old
        return run
    forms = {i: step_as(i) for i in ("kernel", "tensor")}
    out["forms"] = _alternate(forms, a)
    out["peak_bytes"] = {i: _peak(fn) for i, fn in forms.items()}
    return out


def child_trace(a):
    g = _graph("arxiv", a.scale, a)
    forms, _ = _sweeps(g, 128, _operands(g, 128, a))
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    return {"step": "trace", "n_nodes": g.number_of_nodes(), "n_edges": g.number_of_edges(), "F": 128, "calls": 1}


CHILDREN = {
    "op-arxiv-128": lambda a: child_op("arxiv", 128, a.scale, a),
    "op-arxiv-256": lambda a: child_op("arxiv", 256, a.scale, a),
    "op-products-128": lambda a: child_op("products", 128, a.products_scale, a),
    "step-arxiv": child_step,
    "trace": child_trace,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=list(CHILDREN), choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0, help="of S-arxiv")
    ap.add_argument("--products-scale", type=float, default=0.1, help="of S-products where the tensor form runs too")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_gatedgcn.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_gatedgcn.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            tmp = None
            if step == "trace":                    # a run of its own: the kernel trace alone, no counters
                tmp = tempfile.mkdtemp(prefix="bench_gatedgcn_trace_")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + cmd
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [line for line in out.stdout.splitlines() if line.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            if tmp is not None:
                result["kernels"] = _kernel_stats(tmp, os.path.join(os.path.dirname(os.path.abspath(a.out)), "bench_gatedgcn_kernel_stats.csv"))
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
