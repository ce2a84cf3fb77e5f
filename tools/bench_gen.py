"""DeeperGCN (bot_amd.nn.GENConv / DeeperGCN, csrc/spmm_softmax.hip) measured on one GPU.

  kernel-arxiv / kernel-reddit   the softmax sweep forward (`_C.spmm_softmax`, without and with q) against the sum sweep (`_C.spmm` on
            g.csc), the softmax backward (`_C.spmm_softmax_bwd` on g.csr) against the transposed sum sweep (`_C.spmm` on g.csr), and both
            against the tensor form of `ops.copy_u_softmax` (forward; forward + backward) where its [E, F] tensors fit, at F = 256 on
            the workload's graph.  The forms of a group alternate in ONE process: --rounds rounds, each the median of --calls calls
            after --warmup warm-up calls, every call ended by a device synchronise; the spread of a form is its largest minus its
            smallest round.  With the byte models of csrc/spmm_softmax.hip, and the default rule: the kernel form stays the default only
            if it beats the tensor form by more than the tensor form's own spread (`kernel_wins_beyond_tensor_spread`).
  step-NAME   one full-batch train step of `workloads.build_gen(NAME)` beside `workloads.build(NAME)`'s own step, in one process.
  sampled-NAME   one sampled batch (sample + step) of each of the two.
  trace     one `rocprofv3 --kernel-trace --stats` run of a child that calls the sweeps once on S-arxiv (no counters in that run; it is
            for timing only); their rows of the kernel statistics go to bench_gen_kernel_stats.csv beside --out.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_gen.py [--steps kernel-arxiv kernel-reddit step-arxiv sampled-arxiv trace] [--scale 1.0]
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
WIDTH = 256


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
    _ = g.csr
    return g


def _sweeps(g, a):
    """The sweeps as callables over fixed operands, and the sizes."""
    from bot_amd import _C
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(a.seed + 5)
    x = torch.randn(n, WIDTH, generator=gen).to(DEV)
    dout = torch.randn(n, WIDTH, generator=gen).to(DEV)
    beta = torch.ones(1, device=DEV)
    out, lse, q = _C.spmm_softmax(g.csc, x, beta, True, 1e-7, True)
    x3, d3 = x.unsqueeze(1), dout.unsqueeze(1)
    dx = torch.empty_like(x)
    forms = {"softmax_fwd": lambda: _C.spmm_softmax(g.csc, x, beta, True, 1e-7, False, out=out, lse=lse),
             "softmax_fwd_q": lambda: _C.spmm_softmax(g.csc, x, beta, True, 1e-7, True, out=out, lse=lse, q=q),
             "sum_fwd": lambda: _C.spmm(g.csc, x3),
             "softmax_bwd": lambda: _C.spmm_softmax_bwd(g.csr, x, beta, True, 1e-7, dout, out, lse, dx=dx),
             "sum_bwd": lambda: _C.spmm(g.csr, d3)}
    return forms, n, E, x, dout


def _tensor_forms(g, x, dout):
    """The tensor form of the op, forward and forward + backward, or None where its [E, F] tensors do not fit."""
    from bot_amd import ops
    xg = x.clone().requires_grad_()

    def fwd():
        with torch.no_grad():
            return ops.copy_u_softmax(g, x, 1.0, relu=True, eps=1e-7, impl="tensor")

    def fwd_bwd():
        xg.grad = None
        ops.copy_u_softmax(g, xg, 1.0, relu=True, eps=1e-7, impl="tensor").backward(dout)
    try:
        fwd()
        fwd_bwd()
        torch.cuda.synchronize()
    except torch.OutOfMemoryError:
        xg.grad = None
        torch.cuda.empty_cache()
        return None
    return {"tensor_fwd": fwd, "tensor_fwd_bwd": fwd_bwd}


def child_kernel(name, a):
    from bot_amd import ops
    g = _graph(name, a)
    forms, n, E, x, dout = _sweeps(g, a)
    fwd = _alternate({k: forms[k] for k in ("softmax_fwd", "softmax_fwd_q", "sum_fwd")}, a)
    bwd = _alternate({k: forms[k] for k in ("softmax_bwd", "sum_bwd")}, a)
    F = WIDTH
    model = {"sum_fwd": 4 * (E * (1 + F) + n * F), "softmax_fwd": 4 * (E * (1 + F) + 2 * n * F), "softmax_fwd_q": 4 * (E * (1 + F) + 3 * n * F),
             "sum_bwd": 4 * (E * (1 + F) + n * F), "softmax_bwd": 4 * (E * (1 + 3 * F) + 2 * n * F)}
    out = {"step": f"kernel-{name}", "n_nodes": n, "n_edges": E, "F": F, "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup,
           "sum_sweep_path": "blocked" if g.csc.blocked else "rows"}
    for k, v in {**fwd, **bwd}.items():
        v["byte_model"] = model[k]
        v["model_gb_per_s"] = round(model[k] / (v["median_ms"] * 1e-3) / 1e9, 1)
        out[k] = v
    out["fwd_ratio_softmax_over_sum"] = round(fwd["softmax_fwd"]["median_ms"] / fwd["sum_fwd"]["median_ms"], 4)
    out["bwd_ratio_softmax_over_sum"] = round(bwd["softmax_bwd"]["median_ms"] / bwd["sum_bwd"]["median_ms"], 4)
    out["bwd_byte_model_ratio"] = round(model["softmax_bwd"] / model["sum_bwd"], 4)
    tensor = _tensor_forms(g, x, dout)
    if tensor is None:
        out["tensor_form"] = "does not fit"
    else:
        xk = x.clone().requires_grad_()

        def kernel_fwd_bwd():
            xk.grad = None
            ops.copy_u_softmax(g, xk, 1.0, relu=True, eps=1e-7, impl="kernel").backward(dout)
        res = _alternate({"kernel_fwd": forms["softmax_fwd"], "tensor_fwd": tensor["tensor_fwd"], "kernel_fwd_bwd": kernel_fwd_bwd,
                          "tensor_fwd_bwd": tensor["tensor_fwd_bwd"]}, a)
        out["against_tensor_form"] = res
        out["kernel_wins_beyond_tensor_spread"] = {
            "fwd": res["tensor_fwd"]["median_ms"] - res["kernel_fwd"]["median_ms"] > res["tensor_fwd"]["spread_ms"],
            "fwd_bwd": res["tensor_fwd_bwd"]["median_ms"] - res["kernel_fwd_bwd"]["median_ms"] > res["tensor_fwd_bwd"]["spread_ms"]}
        out["tensor_form_peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    out["device"] = torch.cuda.get_device_name(0)
    return out


def child_step(name, a):
    from bot_amd import workloads
    out = {"step": f"step-{name}", "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    for key, make in (("gen", lambda: workloads.build_gen(name, DEV, scale=a.scale, seed=a.seed)),
                      ("build", lambda: workloads.build(name, DEV, scale=a.scale, seed=a.seed))):
        wl = make()
        out["n_nodes"], out["n_edges"] = wl.n_nodes, wl.n_edges
        out[key] = dict(_alternate({"step": wl.step}, a)["step"], describe=wl.describe)
        del wl
        torch.cuda.empty_cache()
    return out


def child_sampled(name, a):
    from bot_amd import workloads
    out = {"step": f"sampled-{name}", "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    for key, make in (("gen", lambda: workloads.build_gen(name, DEV, sampled=True, scale=a.scale, seed=a.seed)),
                      ("build_sampled", lambda: workloads.build_sampled(name, DEV, scale=a.scale, seed=a.seed))):
        wl = make()
        it = [iter(wl.loader)]

        def batch():
            try:
                _, output_nodes, blocks = next(it[0])
            except StopIteration:
                it[0] = iter(wl.loader)
                _, output_nodes, blocks = next(it[0])
            wl.step(blocks, output_nodes)
        out[key] = dict(_alternate({"batch": batch}, a)["batch"], describe=wl.describe)
        del wl
        torch.cuda.empty_cache()
    return out


def child_trace(a):
    g = _graph("arxiv", a)
    forms, n, E, _, _ = _sweeps(g, a)
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    return {"step": "trace", "n_nodes": n, "n_edges": E, "F": WIDTH, "calls": 1}


NAMES = ("cora", "arxiv", "reddit")
CHILDREN = {"trace": child_trace}
for _n in NAMES:
    CHILDREN[f"step-{_n}"] = lambda a, n=_n: child_step(n, a)
    CHILDREN[f"sampled-{_n}"] = lambda a, n=_n: child_sampled(n, a)
for _n in ("arxiv", "reddit"):
    CHILDREN[f"kernel-{_n}"] = lambda a, n=_n: child_kernel(n, a)


def _kernel_stats(directory, out_csv):
    """The sweeps' rows of the run's kernel statistics -> out_csv; returns {kernel: calls and average ns}."""
    import csv
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return {}
    rows = list(csv.DictReader(open(files[0])))
    keep = [r for r in rows if "spmm" in r.get("Name", "")]
    if keep:
        with open(out_csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(keep[0]))
            w.writeheader()
            w.writerows(keep)
    return {r["Name"].split("(")[0].split("::")[-1]: {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"])} for r in keep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=["kernel-arxiv", "kernel-reddit", "step-arxiv", "sampled-arxiv", "trace"],
                    choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_gen.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_gen.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            tmp = None
            if step == "trace":
                tmp = tempfile.mkdtemp(prefix="bench_gen_trace_")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + cmd
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            if tmp is not None:
                result["kernels"] = _kernel_stats(tmp, os.path.join(os.path.dirname(a.out), "bench_gen_kernel_stats.csv"))
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
