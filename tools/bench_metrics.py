"""The on-device evaluator (bot_amd.metrics) measured on one GPU at S-proteins' shape: 132 534 rows x 112 tasks, the workload's own
54 / 18 / 28 % split as three groups, random logits.

  paths     (a) rocauc_counts(impl="kernel"), (b) rocauc_counts(impl="tensor") alternating in ONE process: --rounds rounds, each the
            median of --calls calls after --warmup warm-up calls, every call ended by a device synchronise; the spread of a path is
            its largest minus its smallest round.  (c) the host path, once: device-to-host copy of the predictions plus the numpy
            restatement (tests/metrics_cases.py).  The three must agree integer for integer, or the step fails.
  workload  build_sampled("proteins"): one training epoch beside one wl.evaluate(), and the metric's share of the evaluation (the
            grouped Evaluator call on the predictions, timed on its own).
  trace     one `rocprofv3 --kernel-trace --stats` run of a child that calls the kernel path --calls times (no counters in that
            run); the rocauc_* rows of its kernel statistics go to profiles/bench_metrics_kernel_stats.csv.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_metrics.py [--steps paths workload trace] [--scale 1.0] [--out profiles/bench_metrics.jsonl]
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

N, T = 132534, 112


def _sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def _inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    pred = torch.randn(n, T, generator=gen)
    labels = (torch.rand(n, T, generator=gen) < 0.5).to(torch.int64)
    perm = torch.randperm(n, generator=gen)
    groups = torch.zeros(n, dtype=torch.int8)
    groups[perm[int(0.54 * n):int(0.72 * n)]] = 1
    groups[perm[int(0.72 * n):]] = 2
    return pred, labels, groups


def _median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(calls):
        t0 = _sync()
        fn()
        times.append(_sync() - t0)
    return 1e3 * statistics.median(times)


def child_paths(a):
    import numpy as np

    from bot_amd import metrics
    from tests import metrics_cases as MC
    n = max(8, int(N * a.scale))
    pred, labels, groups = (x.to("cuda:0") for x in _inputs(n, a.seed))
    kernel = lambda: metrics.rocauc_counts(pred, labels, groups, 3, impl="kernel")
    tensor = lambda: metrics.rocauc_counts(pred, labels, groups, 3, impl="tensor")
    rounds = {"kernel": [], "tensor": []}
    for _ in range(a.rounds):                                     # alternating
        rounds["kernel"].append(round(_median_ms(kernel, a.calls, a.warmup), 4))
        rounds["tensor"].append(round(_median_ms(tensor, a.calls, a.warmup), 4))
    t0 = _sync()
    host_pred = pred.cpu().numpy()
    t1 = time.perf_counter()
    ref, _ = MC.counts_reference(host_pred, labels.cpu().numpy(), groups.cpu().numpy(), 3)
    t2 = time.perf_counter()
    if not (np.array_equal(kernel().cpu().numpy(), ref) and np.array_equal(tensor().cpu().numpy(), ref)):
        sys.exit("the three paths disagree")
    out = {"step": "paths", "n": n, "tasks": T, "groups": 3, "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    for k, v in rounds.items():
        out[k] = {"rounds_ms": v, "median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
    out["host"] = {"copy_ms": round(1e3 * (t1 - t0), 2), "restatement_ms": round(1e3 * (t2 - t1), 2), "total_ms": round(1e3 * (t2 - t0), 2)}
    out["kernel_faster_by_ms"] = round(out["tensor"]["median_ms"] - out["kernel"]["median_ms"], 4)
    out["kernel_wins_beyond_tensor_spread"] = out["kernel_faster_by_ms"] > out["tensor"]["spread_ms"]
    out["rocauc"] = [round(v, 6) for v in metrics.rocauc(pred, labels, groups, 3).tolist()]
    out["device"] = torch.cuda.get_device_name(0)
    return out


def child_workload(a):
    from bot_amd import minibatch, workloads
    wl = workloads.build_sampled("proteins", "cuda:0", scale=a.scale, seed=a.seed)
    t0 = _sync()
    loss = wl.epoch()
    t1 = _sync()
    out = wl.evaluate()
    t2 = _sync()
    ds, preds = wl.dataset, out[6]
    n = wl.graph.number_of_nodes()
    groups = minibatch.node_roles(n, ds.train_idx, ds.val_idx, ds.test_idx) - 1
    wl.evaluator.eval_groups(preds, wl.labels, groups, 3)         # warm
    t3 = _sync()
    scores = wl.evaluator.eval_groups(preds, wl.labels, groups, 3)
    t4 = _sync()
    return {"step": "workload", "describe": wl.describe, "n_nodes": n, "eval_fanouts": wl.eval_fanouts, "eval_batch_size": wl.eval_batch_size,
            "eval_batches": len(wl.eval_loader), "train_batches": len(wl.loader), "train_epoch_ms": round(1e3 * (t1 - t0), 2),
            "train_loss": round(loss, 6), "evaluate_ms": round(1e3 * (t2 - t1), 2), "metric_ms": round(1e3 * (t4 - t3), 3),
            "metric_share_of_evaluate": round((t4 - t3) / (t2 - t1), 5), "scores": [round(v, 6) for v in scores],
            "losses": [round(v, 6) for v in out[3:6]], "device": torch.cuda.get_device_name(0)}


def child_trace(a):
    from bot_amd import metrics
    n = max(8, int(N * a.scale))
    pred, labels, groups = (x.to("cuda:0") for x in _inputs(n, a.seed))
    for _ in range(a.calls):
        metrics.rocauc_counts(pred, labels, groups, 3, impl="kernel")
    torch.cuda.synchronize()
    return {"step": "trace", "n": n, "calls": a.calls}


CHILDREN = {"paths": child_paths, "workload": child_workload, "trace": child_trace}


def _kernel_stats(directory, out_csv):
    """The rocauc_* rows of the run's kernel statistics -> out_csv; returns {kernel: average ns}."""
    import csv
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return {}
    rows = list(csv.DictReader(open(files[0])))
    keep = [r for r in rows if "rocauc" in r.get("Name", "")]
    if keep:
        with open(out_csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(keep[0]))
            w.writeheader()
            w.writerows(keep)
    return {r["Name"].split("(")[0].split("::")[-1]: {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"])} for r in keep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=["paths", "workload", "trace"], choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_metrics.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_metrics.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            tmp = None
            if step == "trace":
                tmp = tempfile.mkdtemp(prefix="bench_metrics_trace_")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + cmd
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            if tmp is not None:
                result["kernels"] = _kernel_stats(tmp, os.path.join(os.path.dirname(a.out), "bench_metrics_kernel_stats.csv"))
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
