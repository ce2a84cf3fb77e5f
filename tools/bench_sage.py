"""GraphSAGE (bot_amd.nn.SAGEConv / GraphSAGE, csrc/spmm_max.hip) measured on one GPU.

  kernel-arxiv / kernel-reddit   (a) the max sweep forward (`_C.spmm_max`) against the sum sweep it mirrors (`_C.spmm` on g.csc), and the max
            backward (`_C.spmm_max_bwd` on g.csr + csr2csc) against the transposed sum sweep (`_C.spmm` on g.csr), at F = 256 on the
            workload's graph.  The two of a pair alternate in ONE process: --rounds rounds, each the median of --calls calls after --warmup
            warm-up calls, every call ended by a device synchronise; the spread of a form is its largest minus its smallest round.  With
            the byte models of csrc/spmm_max.hip and the two findings DESIGN §8 asks about: is the forward slower than the sum sweep by
            more than the arg store explains, is the backward slower than twice the transposed sweep plus that sweep's spread.
  fold      one pool layer (256 -> 256 on S-arxiv, forward + backward) with the ReLU folded into the max kernel against
            `relu(fc_pool(h))` as a pass of its own + relu=False, alternating in one process; the fold stays the default only if it
            beats the separate pass by more than that form's spread (`fold_wins_beyond_separate_spread`).
  step-NAME   (b) one full-batch train step of `workloads.build_sage(NAME)` with the mean and with the pool aggregator, beside
            `workloads.build(NAME)`'s own step (cora, arxiv, reddit).
  sampled-NAME   (c) one sampled batch (sample + step) of each of the three.
  trace     one `rocprofv3 --kernel-trace --stats` run of a child that calls the four sweeps of (a) once on S-arxiv (no counters in
            that run); their rows of the kernel statistics go to profiles/bench_sage_kernel_stats.csv.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_sage.py [--steps kernel-arxiv kernel-reddit fold step-arxiv sampled-arxiv trace] [--scale 1.0]
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
    _ = g.csr2csc
    return g


def _sweeps(g, a):
    """The four sweeps of (a) as callables over fixed operands, and the sizes."""
    from bot_amd import _C
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(a.seed + 5)
    x = torch.randn(n, WIDTH, generator=gen).to(DEV)
    dout = torch.randn(n, WIDTH, generator=gen).to(DEV)
    out, arg = _C.spmm_max(g.csc, x)
    x3, d3 = x.unsqueeze(1), dout.unsqueeze(1)
    dx = torch.empty_like(x)
    forms = {"max_fwd": lambda: _C.spmm_max(g.csc, x, False, out=out, arg=arg), "sum_fwd": lambda: _C.spmm(g.csc, x3),
             "max_bwd": lambda: _C.spmm_max_bwd(g.csr, g.csr2csc, dout, arg, out=dx), "sum_bwd": lambda: _C.spmm(g.csr, d3)}
    return forms, n, E


def child_kernel(name, a):
    g = _graph(name, a)
    forms, n, E = _sweeps(g, a)
    fwd = _alternate({k: forms[k] for k in ("max_fwd", "sum_fwd")}, a)
    bwd = _alternate({k: forms[k] for k in ("max_bwd", "sum_bwd")}, a)
    F = WIDTH
    model = {"sum_fwd": 4 * (E * (1 + F) + n * F), "max_fwd": 4 * (E * (1 + F) + 2 * n * F), "sum_bwd": 4 * (E * (1 + F) + n * F),
             "max_bwd": 4 * (E * (2 + 2 * F) + n * F)}
    out = {"step": f"kernel-{name}", "n_nodes": n, "n_edges": E, "F": F, "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup,
           "sum_sweep_path": "blocked" if g.csc.blocked else "rows"}
    for k, v in {**fwd, **bwd}.items():
        v["byte_model"] = model[k]
        v["model_gb_per_s"] = round(model[k] / (v["median_ms"] * 1e-3) / 1e9, 1)
        out[k] = v
    out["fwd_ratio_max_over_sum"] = round(fwd["max_fwd"]["median_ms"] / fwd["sum_fwd"]["median_ms"], 4)
    out["bwd_ratio_max_over_sum"] = round(bwd["max_bwd"]["median_ms"] / bwd["sum_bwd"]["median_ms"], 4)
    # the extra store at the sum sweep's own achieved rate, and the sweep's spread on top
    store_ms = fwd["sum_fwd"]["median_ms"] * (model["max_fwd"] - model["sum_fwd"]) / model["sum_fwd"]
    out["fwd_extra_store_ms_at_sum_rate"] = round(store_ms, 4)
    out["fwd_slower_than_the_store_explains"] = fwd["max_fwd"]["median_ms"] > fwd["sum_fwd"]["median_ms"] + store_ms + fwd["sum_fwd"]["spread_ms"]
    out["bwd_slower_than_twice_sum_plus_spread"] = bwd["max_bwd"]["median_ms"] > 2 * bwd["sum_bwd"]["median_ms"] + bwd["sum_bwd"]["spread_ms"]
    out["device"] = torch.cuda.get_device_name(0)
    return out


def child_fold(a):
    from bot_amd import nn as bnn
    from bot_amd import ops
    g = _graph("arxiv", a)
    n = g.number_of_nodes()
    torch.manual_seed(a.seed)
    conv = bnn.SAGEConv(WIDTH, WIDTH, "pool").to(DEV)
    h = torch.randn(n, WIDTH, device=DEV).requires_grad_()
    dout = torch.randn(n, WIDTH, device=DEV)
    lin = lambda t, fc: ops.linear(t, fc.weight, fc.bias)

    def run(fold):
        conv.zero_grad(set_to_none=True)
        h.grad = None
        z = lin(h, conv.fc_pool)
        m = ops.copy_u_max(g, z, relu=True) if fold else ops.copy_u_max(g, torch.relu(z), relu=False)
        out = lin(h, conv.fc_self) + lin(m, conv.fc_neigh)
        out.backward(dout)
        return out
    diff = (run(True) - run(False)).abs().max().item()
    if not diff <= 1e-5:
        sys.exit(f"the two forms differ by {diff}")
    res = _alternate({"fold": lambda: run(True), "separate": lambda: run(False)}, a)
    out = {"step": "fold", "n_nodes": n, "n_edges": g.number_of_edges(), "F": WIDTH, "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup,
           "max_abs_diff_between_forms": diff, **res}
    out["fold_faster_by_ms"] = round(res["separate"]["median_ms"] - res["fold"]["median_ms"], 4)
    out["fold_wins_beyond_separate_spread"] = out["fold_faster_by_ms"] > res["separate"]["spread_ms"]
    return out


def child_step(name, a):
    from bot_amd import workloads
    out = {"step": f"step-{name}", "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    for key, make in (("sage_mean", lambda: workloads.build_sage(name, DEV, aggregator="mean", scale=a.scale, seed=a.seed)),
                      ("sage_pool", lambda: workloads.build_sage(name, DEV, aggregator="pool", scale=a.scale, seed=a.seed)),
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
    for key, make in (("sage_mean", lambda: workloads.build_sage(name, DEV, aggregator="mean", sampled=True, scale=a.scale, seed=a.seed)),
                      ("sage_pool", lambda: workloads.build_sage(name, DEV, aggregator="pool", sampled=True, scale=a.scale, seed=a.seed)),
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
    forms, n, E = _sweeps(g, a)
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    return {"step": "trace", "n_nodes": n, "n_edges": E, "F": WIDTH, "calls": 1}


NAMES = ("cora", "arxiv", "reddit")
CHILDREN = {"fold": child_fold, "trace": child_trace}
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
    ap.add_argument("--steps", nargs="+", default=["kernel-arxiv", "kernel-reddit", "fold", "step-arxiv", "sampled-arxiv", "trace"],
                    choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sage.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_sage.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            tmp = None
            if step == "trace":
                tmp = tempfile.mkdtemp(prefix="bench_sage_trace_")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + cmd
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            if tmp is not None:
                result["kernels"] = _kernel_stats(tmp, os.path.join(os.path.dirname(a.out), "bench_sage_kernel_stats.csv"))
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
