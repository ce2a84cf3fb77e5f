"""Correct and Smooth (bot_amd.smoothing) measured on one GPU on the graphs of S-arxiv (40 classes) and S-products (47 classes): the
default 50 + 50 iterations on a random softmax, the workload's 54 % training split as the labelled rows.

  arxiv / products   (a) CorrectAndSmooth(impl="kernel"), (b) CorrectAndSmooth(impl="tensor") alternating in ONE process: --rounds rounds,
            each the median of --calls calls after --warmup warm-up calls, every call ended by a device synchronise; the spread of a form
            is its largest minus its smallest round.  The two forms must agree to 1e-5, or the step fails.  Per iteration (a call's time
            over its 100 sweeps, glue included) the achieved rate against the byte model E (4 + 4 + 4 C) + 3 N 4 C.
  trace     one `rocprofv3 --kernel-trace --stats` run of a child that calls the kernel form once on S-arxiv (no counters in that run);
            the prop_* rows of its kernel statistics go to profiles/bench_smooth_kernel_stats.csv.

--edge-weight: the same steps with per-edge weights (seeded uniform in [0.5, 1.5), handed over as a tensor in edge-id order): the weighted
kernel form (`bot_propagate_step_w_f32`, one more streamed word per edge in the byte model) against the weighted tensor form, into
profiles/bench_smooth_weighted.jsonl and profiles/bench_smooth_weighted_kernel_stats.csv.  The rule the figures decide: the weighted kernel
form stays `smoothing.default_impl`'s answer with a weight only if it beats the weighted tensor form by more than that form's
round-to-round spread (`kernel_wins_beyond_tensor_spread`); otherwise `smoothing.WEIGHTED_KERNEL` is set to False.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_smooth.py [--steps arxiv products trace] [--scale 1.0] [--out profiles/bench_smooth.jsonl]
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


def _inputs(name, a):
    """The workload's graph (the same seeded edges and preprocessing as bot_amd.workloads) without its feature matrix."""
    import bot_amd
    from bot_amd import synth
    n, e_raw, _, C = synth.SHAPES[name]
    n, e_raw = max(8, int(n * a.scale)), max(8, int(e_raw * a.scale))
    s, d = synth.powerlaw_edges(n, e_raw, synth.BASE_SEED + a.seed, device="cuda:0")
    g = bot_amd.preprocess(bot_amd.Graph(s, d, n))
    gen = torch.Generator().manual_seed(synth.BASE_SEED + 1000 + a.seed)
    y_soft = torch.softmax(torch.randn(n, C, generator=gen), dim=-1).to("cuda:0")
    labels = torch.randint(0, C, (n,), generator=gen).to("cuda:0")
    mask = torch.randperm(n, generator=gen)[:int(0.54 * n)].to("cuda:0")
    return g, y_soft, labels[mask], mask, C


def _weight(g, a):
    """--edge-weight: float32 [E] on the device, seeded uniform in [0.5, 1.5); None without the flag."""
    if not a.edge_weight:
        return None
    gen = torch.Generator().manual_seed(a.seed + 77)
    return (0.5 + torch.rand(g.number_of_edges(), generator=gen)).to("cuda:0")


def child_forms(name, a):
    from bot_amd import smoothing
    g, y_soft, y_true, mask, C = _inputs(name, a)
    w = _weight(g, a)
    kw = {} if w is None else {"edge_weight": w}
    forms = {k: smoothing.CorrectAndSmooth(impl=k) for k in ("kernel", "tensor")}
    run = {k: (lambda cs=cs: cs(g, y_soft, y_true, mask, **kw)) for k, cs in forms.items()}
    diff = (run["kernel"]() - run["tensor"]()).abs().max().item()
    if not diff <= 1e-5:
        sys.exit(f"the two forms differ by {diff}")
    rounds = {"kernel": [], "tensor": []}
    for _ in range(a.rounds):                                     # alternating
        for k in rounds:
            rounds[k].append(round(_median_ms(run[k], a.calls, a.warmup), 4))
    n, E = g.number_of_nodes(), g.number_of_edges()
    sweeps = forms["kernel"].num_correction_layers + forms["kernel"].num_smoothing_layers
    model = E * (4 + 4 + 4 * C + (4 if w is not None else 0)) + 3 * n * 4 * C
    out = {"step": name, "edge_weight": w is not None, "n_nodes": n, "n_edges": E, "classes": C, "sweeps": sweeps, "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup,
           "byte_model_per_sweep": model, "max_abs_diff_between_forms": diff}
    for k, v in rounds.items():
        med = statistics.median(v)
        out[k] = {"rounds_ms": v, "median_ms": round(med, 4), "spread_ms": round(max(v) - min(v), 4), "ms_per_sweep": round(med / sweeps, 5),
                  "model_gb_per_s": round(model / (med / sweeps * 1e-3) / 1e9, 1)}
    out["kernel_faster_by_ms"] = round(out["tensor"]["median_ms"] - out["kernel"]["median_ms"], 4)
    out["kernel_wins_beyond_tensor_spread"] = out["kernel_faster_by_ms"] > out["tensor"]["spread_ms"]
    out["device"] = torch.cuda.get_device_name(0)
    return out


def child_trace(a):
    from bot_amd import smoothing
    g, y_soft, y_true, mask, C = _inputs("arxiv", a)
    cs = smoothing.CorrectAndSmooth(impl="kernel")
    w = _weight(g, a)
    cs(g, y_soft, y_true, mask, **({} if w is None else {"edge_weight": w}))
    torch.cuda.synchronize()
    return {"step": "trace", "edge_weight": w is not None, "n_nodes": g.number_of_nodes(), "n_edges": g.number_of_edges(), "classes": C, "calls": 1}


CHILDREN = {"arxiv": lambda a: child_forms("arxiv", a), "products": lambda a: child_forms("products", a), "trace": child_trace}


def _kernel_stats(directory, out_csv):
    """The prop_* rows of the run's kernel statistics -> out_csv; returns {kernel: calls and average ns}."""
    import csv
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return {}
    rows = list(csv.DictReader(open(files[0])))
    keep = [r for r in rows if "prop_" in r.get("Name", "")]
    if keep:
        with open(out_csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(keep[0]))
            w.writeheader()
            w.writerows(keep)
    return {r["Name"].split("(")[0].split("::")[-1]: {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"])} for r in keep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=["arxiv", "products", "trace"], choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step's child process may run")
    ap.add_argument("--edge-weight", action="store_true", help="weighted kernel form against weighted tensor form")
    ap.add_argument("--out", default=None, help="default profiles/bench_smooth.jsonl (bench_smooth_weighted.jsonl with --edge-weight)")
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_smooth.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    tag = "bench_smooth_weighted" if a.edge_weight else "bench_smooth"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", tag + ".jsonl")
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            tmp = None
            if step == "trace":
                tmp = tempfile.mkdtemp(prefix="bench_smooth_trace_")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + cmd
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            if tmp is not None:
                result["kernels"] = _kernel_stats(tmp, os.path.join(os.path.dirname(a.out), tag + "_kernel_stats.csv"))
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
