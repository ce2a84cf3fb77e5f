"""PNA (bot_amd.ops.pna_aggregate, csrc/spmm_pna.hip) measured on one GPU.

  agg-NAME-F   (NAME arxiv / reddit, F 64 / 256) the aggregation with 4 aggregators (mean, max, min, std) x 3 scalers (identity,
            amplification, attenuation), delta = nn.pna_delta of the graph, a [n, F] and b [n, F] seeded normal, on the workload's
            graph.  The fused sweep (impl="kernel") and the tensor form (impl="tensor": sum sweeps over a and a * a, max sweeps over a
            and -a, dense ops) alternate in ONE process: --rounds rounds, each the median of --calls calls after --warmup warm-up
            calls, every call ended by a device synchronise; the spread of a form is its largest minus its smallest round.  Timed:
            the forward alone (no gradient asked for), and forward + backward (gradients of a and b).  The standing rule: the kernel
            form is the default only if it beats the tensor form by more than the tensor form's own spread
            (`kernel_wins_beyond_tensor_spread`, both timings).
            The pivot's price: the raw forward sweep (`_C.spmm_pna`, saved arrays off) with the pivot at the row's first neighbour -
            a gather of one more random row per item - against the same sweep with the pivot pointed at a's row 0, a constant row
            that stays in the cache, alternating the same way (`pivot_price_ms`, beside the constant-row form's spread).
            Byte models (4-byte words; E edges, n rows, W = 12 F output columns, R = 7 F record words):
              forward           4 * [E * (1 + F) + n * (W + F)]            ids and source rows per edge; the output row and b per row
              forward, saving   + 4 * n * 4 F                              the mean, the std and the two position arrays
              backward          4 * [n * (W + 4 F + R + F)]                the dense pass: dout, saved, the record, db
                                + 4 * [E * (2 + R) + 2 * n * F]            ids, positions and a record per edge; a and da per row
            `model_gb_per_s` is the model's bytes over the median time: a rate of the MODEL, above the HBM rate where the gathered rows
            hit in the Infinity Cache.
  trace     one `rocprofv3 --kernel-trace --stats` run of a child that calls the kernel form's forward + backward once at F = 256 on
            S-arxiv (no counters in that run); the PNA kernels' rows go to bench_pna_kernel_stats.csv beside --out.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_pna.py [--steps agg-arxiv-64 agg-arxiv-256 agg-reddit-64 agg-reddit-256 trace] [--scale 1.0]
"""
import argparse
import glob
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

DEV = "cuda:0"
AGGS = ("mean", "max", "min", "std")
SCALERS = ("identity", "amplification", "attenuation")


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


def _graph(name, a):
    """The workload's graph (the same seeded edges and preprocessing as bot_amd.workloads) without its feature matrix."""
    import bot_amd
    from bot_amd import synth
    n, e_raw, _, _ = synth.SHAPES[name]
    n, e_raw = max(8, int(n * a.scale)), max(8, int(e_raw * a.scale))
    s, d = synth.powerlaw_edges(n, e_raw, synth.BASE_SEED + a.seed, device=DEV)
    g = bot_amd.preprocess(bot_amd.Graph(s, d, n))
    _ = g.csr2csc
    return g


def _operands(g, F, a):
    from bot_amd import nn as bnn
    n = g.number_of_nodes()
    gen = torch.Generator().manual_seed(a.seed + 5)
    x = torch.randn(n, F, generator=gen).to(DEV)
    b = torch.randn(n, F, generator=gen).to(DEV)
    dout = torch.randn(n, len(AGGS) * len(SCALERS) * F, generator=gen).to(DEV)
    return x, b, dout, bnn.pna_delta(g)


def _forms(g, x, b, dout, delta):
    from bot_amd import ops

    def fwd(impl):
        with torch.no_grad():
            return ops.pna_aggregate(g, x, b, AGGS, SCALERS, delta, impl=impl)

    def both(impl):
        xa, ba = x.detach().requires_grad_(), b.detach().requires_grad_()
        out = ops.pna_aggregate(g, xa, ba, AGGS, SCALERS, delta, impl=impl)
        out.backward(dout)
        return out, xa.grad, ba.grad
    return fwd, both


def child_agg(name, F, a):
    from bot_amd import _C, ops
    g = _graph(name, a)
    n, E = g.number_of_nodes(), g.number_of_edges()
    x, b, dout, delta = _operands(g, F, a)
    fwd, both = _forms(g, x, b, dout, delta)
    ok, ot = both("kernel"), both("tensor")
    diffs = [float((p.detach() - q.detach()).abs().max() / q.detach().abs().max().clamp(min=1e-30)) for p, q in zip(ok, ot)]
    # out and db agree to rounding.  da: where two neighbours of a row are nearly equal the tensor form's raw moments
    # (mean a^2 - mean(a)^2 in float32) lose the small variance and with it the std gradient, an O(1) error in a few entries that the
    # kernel's pivoted moments do not make; the bound here only catches a broken form.
    if not (diffs[0] <= 1e-3 and diffs[2] <= 1e-3 and diffs[1] <= 5e-2):
        sys.exit(f"the two forms differ: {diffs}")
    del ok, ot
    res_f = _alternate({"kernel": lambda: fwd("kernel"), "tensor": lambda: fwd("tensor")}, a)
    res_b = _alternate({"kernel": lambda: both("kernel"), "tensor": lambda: both("tensor")}, a)
    scale = ops.pna_scale_table(g, SCALERS, delta)
    out = torch.empty((n, 12 * F), device=DEV)
    piv = _alternate({"first_neighbour": lambda: _C.spmm_pna(g.csc, x, b, AGGS, scale, F, pivot=True, out=out),
                      "constant_row": lambda: _C.spmm_pna(g.csc, x, b, AGGS, scale, F, pivot=False, out=out)}, a)
    W, R = 12 * F, 7 * F
    m_fwd = 4 * (E * (1 + F) + n * (W + F))
    m_bwd = 4 * (n * (W + 4 * F + R + F)) + 4 * (E * (2 + R) + 2 * n * F)
    res = {"step": f"agg-{name}-{F}", "n_nodes": n, "n_edges": E, "F": F, "aggregators": AGGS, "scalers": SCALERS, "delta": round(delta, 4),
           "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "max_rel_diff_between_forms_out_da_db": [float(f"{d:.3g}") for d in diffs],
           "kernel_instance": None, "forward": res_f, "forward_backward": res_b, "pivot": piv}
    fwd("kernel")
    res["kernel_instance"] = _C._lib.bot_last_kernel().decode()
    res_f["kernel"]["byte_model"], res_b["kernel"]["byte_model"] = m_fwd, m_fwd + 4 * n * 4 * F + m_bwd
    piv["first_neighbour"]["byte_model"] = piv["constant_row"]["byte_model"] = m_fwd
    for v in (res_f["kernel"], res_b["kernel"], piv["first_neighbour"], piv["constant_row"]):
        v["model_gb_per_s"] = round(v["byte_model"] / (v["median_ms"] * 1e-3) / 1e9, 1)
    for key, r in (("forward", res_f), ("forward_backward", res_b)):
        res[f"{key}_kernel_faster_by_ms"] = round(r["tensor"]["median_ms"] - r["kernel"]["median_ms"], 4)
        res[f"{key}_speedup"] = round(r["tensor"]["median_ms"] / r["kernel"]["median_ms"], 3)
        res[f"{key}_kernel_wins_beyond_tensor_spread"] = res[f"{key}_kernel_faster_by_ms"] > r["tensor"]["spread_ms"]
    res["pivot_price_ms"] = round(piv["first_neighbour"]["median_ms"] - piv["constant_row"]["median_ms"], 4)
    res["pivot_price_percent"] = round(100 * res["pivot_price_ms"] / piv["constant_row"]["median_ms"], 2)
    res["device"] = torch.cuda.get_device_name(0)
    return res


def child_trace(a):
    g = _graph("arxiv", a)
    x, b, dout, delta = _operands(g, 256, a)
    _, both = _forms(g, x, b, dout, delta)
    both("kernel")
    torch.cuda.synchronize()
    return {"step": "trace", "n_nodes": g.number_of_nodes(), "n_edges": g.number_of_edges(), "F": 256, "calls": 1}


CHILDREN = {"trace": child_trace}
for _n in ("arxiv", "reddit"):
    for _f in (64, 256):
        CHILDREN[f"agg-{_n}-{_f}"] = lambda a, n=_n, f=_f: child_agg(n, f, a)


def _kernel_stats(directory, out_csv):
    """The PNA kernels' rows of the run's kernel statistics -> out_csv; returns {kernel: calls and average ns}."""
    import csv
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return {}
    rows = list(csv.DictReader(open(files[0])))
    keep = [r for r in rows if "pna" in r.get("Name", "")]
    if keep:
        with open(out_csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(keep[0]))
            w.writeheader()
            w.writerows(keep)
    return {r["Name"].split("(")[0].split("::")[-1]: {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"])} for r in keep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=["agg-arxiv-64", "agg-arxiv-256", "agg-reddit-64", "agg-reddit-256", "trace"],
                    choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pna.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_pna.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            tmp = None
            if step == "trace":
                tmp = tempfile.mkdtemp(prefix="bench_pna_trace_")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + cmd
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            if tmp is not None:
                result["kernels"] = _kernel_stats(tmp, os.path.join(os.path.dirname(a.out), "bench_pna_kernel_stats.csv"))
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
