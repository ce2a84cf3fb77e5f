"""DeeperGCN with raw edge features (bot_amd.nn.GENConv(edge_dim=), csrc/spmm_softmax_edge.hip) measured on one GPU.

  kernel-proteins-64 / kernel-proteins-256 / kernel-arxiv-256   the edge-feature sweeps at K = 8 on the workload's graph at --scale:
            forward without and with q (`_C.spmm_softmax_edge`) beside `_C.spmm_softmax`, backward with and without dweight
            (`_C.spmm_softmax_edge_bwd`) beside `_C.spmm_softmax_bwd`, same graph and width.  The forms of a group alternate in ONE
            process: --rounds rounds, each the median of --calls calls after --warmup warm-up calls, every call ended by a device
            synchronise; the spread of a form is its largest minus its smallest round.  With both byte models (the file headers').
  tensor-proteins   `ops.u_add_e_softmax` (forward; forward + backward with every gradient) in its kernel form against its tensor form at
            F = 256, K = 8 at the largest S-proteins scale of --tensor-scales at which the tensor form fits (each scale is tried, largest
            first, and the ones that ran out of memory are recorded), with the peak allocated memory of both forms and the default rule:
            the kernel form stays the default only if it beats the tensor form by more than the tensor form's own spread.
  step-proteins      one full-batch step of `workloads.build_gen_edge("proteins")` beside `workloads.build("proteins")`'s, one process.
  sampled-proteins   one sampled batch (sample + step) of `build_gen_edge("proteins", sampled=True)` beside `build_sampled("proteins")`.
  trace     one `rocprofv3 --kernel-trace --stats` run of a child that calls the sweeps once on S-arxiv (no counters in that run; it is
            for timing only); their rows of the kernel statistics go to bench_gen_edge_kernel_stats.csv beside --out.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_gen_edge.py [--steps kernel-proteins-256 tensor-proteins step-proteins trace] [--scale 1.0]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_gen import DEV, _alternate, _kernel_stats  # noqa: E402

K = 8


def _graph(name, a, scale=None):
    """(graph, raw edge features [E, K]) of the workload: the seeded edges and preprocessing of bot_amd.workloads; S-proteins with its own
    8 edge features, S-arxiv with 8 seeded uniform ones."""
    import bot_amd
    from bot_amd import synth, workloads
    scale = a.scale if scale is None else scale
    if name == "proteins":
        ds = workloads._edge_dataset(name, torch.device(DEV), a.seed, scale)
        g, ef = ds.graph, ds.efeat
    else:
        n, e_raw, _, _ = synth.SHAPES[name]
        n, e_raw = max(8, int(n * scale)), max(8, int(e_raw * scale))
        s, d = synth.powerlaw_edges(n, e_raw, synth.BASE_SEED + a.seed, device=DEV)
        g = bot_amd.preprocess(bot_amd.Graph(s, d, n))
        ef = torch.rand(g.number_of_edges(), K, generator=torch.Generator().manual_seed(a.seed + 7)).to(DEV)
    _ = g.csr
    return g, ef.contiguous()


def _operands(g, F, a):
    gen = torch.Generator().manual_seed(a.seed + 5)
    n = g.number_of_nodes()
    x, dout = torch.randn(n, F, generator=gen).to(DEV), torch.randn(n, F, generator=gen).to(DEV)
    w, b = (torch.randn(F, K, generator=gen) / K ** 0.5).to(DEV), torch.randn(F, generator=gen).to(DEV)
    return x, dout, w, b


def _sweeps(g, ef, F, a):
    from bot_amd import _C, ops
    x, dout, w, b = _operands(g, F, a)
    beta = torch.ones(1, device=DEV)
    rows = ops._csc_edge_rows(g)
    out, lse, q = _C.spmm_softmax_edge(g.csc, x, ef, w, b, beta, True, 1e-7, True, eperm=rows)
    dx = torch.empty_like(x)
    n_items = g.csr.n_items
    ws = torch.empty(min(1024, n_items // 16 + 1) * K * F, device=DEV)
    return {"edge_fwd": lambda: _C.spmm_softmax_edge(g.csc, x, ef, w, b, beta, True, 1e-7, False, eperm=rows, out=out, lse=lse),
            "edge_fwd_q": lambda: _C.spmm_softmax_edge(g.csc, x, ef, w, b, beta, True, 1e-7, True, eperm=rows, out=out, lse=lse, q=q),
            "softmax_fwd": lambda: _C.spmm_softmax(g.csc, x, beta, True, 1e-7, False, out=out, lse=lse),
            "softmax_fwd_q": lambda: _C.spmm_softmax(g.csc, x, beta, True, 1e-7, True, out=out, lse=lse, q=q),
            "edge_bwd_dw": lambda: _C.spmm_softmax_edge_bwd(g.csr, x, ef, w, b, beta, True, 1e-7, dout, out, lse, eperm=g.csr.eid, dx=dx,
                                                            dw_workspace=ws),
            "edge_bwd": lambda: _C.spmm_softmax_edge_bwd(g.csr, x, ef, w, b, beta, True, 1e-7, dout, out, lse, eperm=g.csr.eid, dx=dx,
                                                         want_dweight=False),
            "softmax_bwd": lambda: _C.spmm_softmax_bwd(g.csr, x, beta, True, 1e-7, dout, out, lse, dx=dx)}


def child_kernel(name, F, a):
    g, ef = _graph(name, a)
    n, E = g.number_of_nodes(), g.number_of_edges()
    forms = _sweeps(g, ef, F, a)
    res = _alternate({k: forms[k] for k in ("edge_fwd", "edge_fwd_q", "softmax_fwd", "softmax_fwd_q")}, a)
    res.update(_alternate({k: forms[k] for k in ("edge_bwd_dw", "edge_bwd", "softmax_bwd")}, a))
    from bot_amd import ops
    perm = ops._csc_edge_rows(g) is not None                 # the positions' edge ids are streamed too: 4 E bytes beside the model's
    model = {"edge_fwd": 4 * (E * (1 + K + F) + 2 * n * F), "edge_fwd_q": 4 * (E * (1 + K + F) + 3 * n * F),
             "softmax_fwd": 4 * (E * (1 + F) + 2 * n * F), "softmax_fwd_q": 4 * (E * (1 + F) + 3 * n * F),
             "edge_bwd_dw": 4 * (E * (2 + K + 3 * F) + 2 * n * F), "edge_bwd": 4 * (E * (2 + K + 3 * F) + 2 * n * F),
             "softmax_bwd": 4 * (E * (1 + 3 * F) + 2 * n * F)}
    out = {"step": f"kernel-{name}-{F}", "n_nodes": n, "n_edges": E, "F": F, "K": K, "scale": a.scale, "rounds": a.rounds, "calls": a.calls,
           "warmup": a.warmup, "eperm_streamed": bool(perm)}
    for k, v in res.items():
        v["byte_model"] = model[k]
        v["model_gb_per_s"] = round(model[k] / (v["median_ms"] * 1e-3) / 1e9, 1)
        out[k] = v
    out["fwd_ratio_edge_over_softmax"] = round(res["edge_fwd"]["median_ms"] / res["softmax_fwd"]["median_ms"], 4)
    out["bwd_ratio_edge_over_softmax"] = round(res["edge_bwd"]["median_ms"] / res["softmax_bwd"]["median_ms"], 4)
    out["bwd_dweight_cost_ms"] = round(res["edge_bwd_dw"]["median_ms"] - res["edge_bwd"]["median_ms"], 4)
    out["device"] = torch.cuda.get_device_name(0)
    return out


def _op_forms(g, ef, F, a, impl):
    from bot_amd import ops
    x, dout, w, b = _operands(g, F, a)
    xg, wg, bg = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()

    def fwd():
        with torch.no_grad():
            return ops.u_add_e_softmax(g, x, ef, w, b, 1.0, relu=True, eps=1e-7, impl=impl)

    def fwd_bwd():
        xg.grad = wg.grad = bg.grad = None
        ops.u_add_e_softmax(g, xg, ef, wg, bg, 1.0, relu=True, eps=1e-7, impl=impl).backward(dout)
    return fwd, fwd_bwd


def child_tensor(a):
    out = {"step": "tensor-proteins", "F": a.tensor_width, "K": K, "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "scales_tried": {}}
    for scale in sorted(a.tensor_scales, reverse=True):
        g, ef = _graph("proteins", a, scale)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t_fwd, t_fwd_bwd = _op_forms(g, ef, a.tensor_width, a, "tensor")
        try:
            t_fwd()
            t_fwd_bwd()
            torch.cuda.synchronize()
        except torch.OutOfMemoryError:
            out["scales_tried"][str(scale)] = "the tensor form ran out of memory"
            del g, ef, t_fwd, t_fwd_bwd
            torch.cuda.empty_cache()
            continue
        except (RuntimeError, ValueError) as e:                    # e.g. the 2^24-edge limit of the tensor form's gather
            out["scales_tried"][str(scale)] = f"the tensor form refused: {type(e).__name__}: {str(e)[:120]}"
            del g, ef, t_fwd, t_fwd_bwd
            torch.cuda.empty_cache()
            continue
        out["scales_tried"][str(scale)] = "fits"
        out["scale"], out["n_nodes"], out["n_edges"] = scale, g.number_of_nodes(), g.number_of_edges()
        out["tensor_form_peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        k_fwd, k_fwd_bwd = _op_forms(g, ef, a.tensor_width, a, "kernel")
        k_fwd()
        k_fwd_bwd()
        torch.cuda.synchronize()
        out["kernel_form_peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
        res = _alternate({"kernel_fwd": k_fwd, "tensor_fwd": t_fwd, "kernel_fwd_bwd": k_fwd_bwd, "tensor_fwd_bwd": t_fwd_bwd}, a)
        out["against_tensor_form"] = res
        out["kernel_wins_beyond_tensor_spread"] = {
            "fwd": res["tensor_fwd"]["median_ms"] - res["kernel_fwd"]["median_ms"] > res["tensor_fwd"]["spread_ms"],
            "fwd_bwd": res["tensor_fwd_bwd"]["median_ms"] - res["kernel_fwd_bwd"]["median_ms"] > res["tensor_fwd_bwd"]["spread_ms"]}
        break
    out["device"] = torch.cuda.get_device_name(0)
    return out


def child_step(a):
    from bot_amd import workloads
    out = {"step": "step-proteins", "scale": a.scale, "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    for key, make in (("gen_edge", lambda: workloads.build_gen_edge("proteins", DEV, scale=a.scale, seed=a.seed)),
                      ("build", lambda: workloads.build("proteins", DEV, scale=a.scale, seed=a.seed))):
        wl = make()
        out["n_nodes"], out["n_edges"] = wl.n_nodes, wl.n_edges
        torch.cuda.reset_peak_memory_stats()
        out[key] = dict(_alternate({"step": wl.step}, a)["step"], describe=wl.describe, peak_gb=round(torch.cuda.max_memory_allocated() / 1e9, 2))
        del wl
        torch.cuda.empty_cache()
    return out


def child_sampled(a):
    from bot_amd import workloads
    out = {"step": "sampled-proteins", "scale": a.scale, "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    for key, make in (("gen_edge", lambda: workloads.build_gen_edge("proteins", DEV, sampled=True, scale=a.scale, seed=a.seed)),
                      ("build_sampled", lambda: workloads.build_sampled("proteins", DEV, scale=a.scale, seed=a.seed))):
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
    g, ef = _graph("arxiv", a)
    for fn in _sweeps(g, ef, 256, a).values():
        fn()
    torch.cuda.synchronize()
    return {"step": "trace", "n_nodes": g.number_of_nodes(), "n_edges": g.number_of_edges(), "F": 256, "K": K, "calls": 1}


CHILDREN = {"kernel-proteins-64": lambda a: child_kernel("proteins", 64, a), "kernel-proteins-256": lambda a: child_kernel("proteins", 256, a),
            "kernel-arxiv-256": lambda a: child_kernel("arxiv", 256, a), "tensor-proteins": child_tensor, "step-proteins": child_step,
            "sampled-proteins": child_sampled, "trace": child_trace}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=list(CHILDREN), choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--tensor-scales", type=float, nargs="+", default=[1.0, 0.5, 0.25, 0.125, 0.0625])
    ap.add_argument("--tensor-width", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_gen_edge.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_gen_edge.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            tmp = None
            if step == "trace":
                tmp = tempfile.mkdtemp(prefix="bench_gen_edge_trace_")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + cmd
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            if tmp is not None:
                result["kernels"] = _kernel_stats(tmp, os.path.join(os.path.dirname(os.path.abspath(a.out)), "bench_gen_edge_kernel_stats.csv"))
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
