"""`ops.appnp_propagate` (bot_amd/appnp.py, csrc/appnp.hip) measured on one GPU on the graphs of S-arxiv (C = 40), S-reddit (C = 41, run
padded to 44) and S-products (C = 47, padded to 48), and one train step of the two workloads built on it.

  arxiv / reddit / products   k = 10, forward + backward of `appnp_propagate` alone on random logits, at edge_drop 0 and 0.5:
            (a) impl="kernel", (b) impl="tensor" alternating in ONE process: --rounds rounds, each the median of --calls calls after
            --warmup warm-up calls, every call ended by a device synchronise; the spread of a form is its largest minus its smallest
            round.  Per form `torch.cuda.max_memory_allocated` over one call above what is allocated before it, and per sweep (a call is
            2 k sweeps) the achieved rate against the byte model of csrc/appnp.hip,
            4 [E_kept C + E (1 + [src_scale] + [ew] + [pos]) + N C (1 + [y0] + 2 [acc])], averaged over the call's sweeps.
            The two forms must agree to 1e-4 of the largest entry, or the step fails.
  models    one `workloads.build_appnp("arxiv")` step and one `workloads.build_gcn2("arxiv")` step, median ms of --calls.

The rule the figures decide: impl=None selects the kernel form at a setting (edge_drop 0 / > 0) only if it beats the tensor form there by
more than that form's round-to-round spread (`kernel_wins_beyond_tensor_spread`) on every graph measured; otherwise
`bot_amd.appnp.KERNEL_DEFAULT` is switched off for that setting.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_appnp.py [--steps arxiv reddit products models] [--scale 1.0] [--out profiles/bench_appnp.jsonl]
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

K = 10
ALPHA = 0.1


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


def _graph(name, a):
    """The workload's graph (the same seeded edges and preprocessing as bot_amd.workloads) without its feature matrix."""
    import bot_amd
    from bot_amd import synth
    n, e_raw, _, C = synth.SHAPES[name]
    n, e_raw = max(8, int(n * a.scale)), max(8, int(e_raw * a.scale))
    s, d = synth.powerlaw_edges(n, e_raw, synth.BASE_SEED + a.seed, device="cuda:0")
    g = bot_amd.preprocess(bot_amd.Graph(s, d, n))
    g.create_formats_()
    return g, C


def _byte_model(n, E, Cp, p):
    """Bytes of one call's 2 k sweeps by the model of csrc/appnp.hip's header (the op's plan: src_scale per edge on the first sweep of a
    direction only, y0 on every forward sweep and on the last backward one, acc on the k - 1 first backward sweeps, pos when p > 0)."""
    kept = E * (1.0 - p)
    fwd = K * (kept * Cp + E + n * Cp * 2) + E
    bwd = K * (kept * Cp + E * (2 if p > 0 else 1) + n * Cp) + E + (K - 1) * 2 * n * Cp + n * Cp
    return 4 * (fwd + bwd)


def child_forms(name, a):
    from bot_amd import ops
    g, C = _graph(name, a)
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(a.seed + 5)
    x = torch.randn(n, C, generator=gen).to("cuda:0").requires_grad_()
    dout = torch.randn(n, C, generator=gen).to("cuda:0")
    Cp = C if C % 4 == 0 else C + 4 - C % 4
    out = {"step": name, "n_nodes": n, "n_edges": E, "classes": C, "width_run": Cp, "k": K, "alpha": ALPHA, "rounds": a.rounds, "calls": a.calls,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "settings": {}}
    for p in (0.0, 0.5):
        def call(impl):
            x.grad = None
            y = ops.appnp_propagate(g, x, K, ALPHA, edge_drop=p, seed=12345, impl=impl)
            y.backward(dout)
            return y.detach(), x.grad
        (yk, gk), (yt, gt) = call("kernel"), call("tensor")
        diff = max(float((yk - yt).abs().max() / yt.abs().max()), float((gk - gt).abs().max() / gt.abs().max()))
        if not diff <= 1e-4:
            sys.exit(f"{name} edge_drop={p}: the two forms differ by {diff} of the largest entry")
        del yk, gk, yt, gt
        res = {"max_rel_diff_between_forms": diff, "byte_model_per_call": _byte_model(n, E, Cp, p)}
        rounds = {"kernel": [], "tensor": []}
        for _ in range(a.rounds):                                     # alternating
            for impl in rounds:
                rounds[impl].append(round(_median_ms(lambda: call(impl), a.calls, a.warmup), 4))
        for impl, v in rounds.items():
            x.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            call(impl)
            torch.cuda.synchronize()
            med = statistics.median(v)
            res[impl] = {"rounds_ms": v, "median_ms": round(med, 4), "spread_ms": round(max(v) - min(v), 4),
                         "peak_extra_mb": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)}
        res["kernel"]["model_gb_per_s"] = round(res["byte_model_per_call"] / (res["kernel"]["median_ms"] * 1e-3) / 1e9, 1)
        res["kernel_faster_by_ms"] = round(res["tensor"]["median_ms"] - res["kernel"]["median_ms"], 4)
        res["kernel_wins_beyond_tensor_spread"] = res["kernel_faster_by_ms"] > res["tensor"]["spread_ms"]
        out["settings"][f"edge_drop_{p}"] = res
    return out


def child_models(a):
    from bot_amd import workloads
    out = {"step": "models", "scale": a.scale, "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for tag, build in (("appnp_arxiv_step_ms", workloads.build_appnp), ("gcn2_arxiv_step_ms", workloads.build_gcn2)):
        wl = build("arxiv", "cuda:0", scale=a.scale, seed=a.seed)
        out[tag] = round(_median_ms(wl.step, a.calls, a.warmup), 3)
        del wl
        torch.cuda.empty_cache()
    return out


CHILDREN = {"arxiv": lambda a: child_forms("arxiv", a), "reddit": lambda a: child_forms("reddit", a),
            "products": lambda a: child_forms("products", a), "models": child_models}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=["arxiv", "reddit", "models"], choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_appnp.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_appnp.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
