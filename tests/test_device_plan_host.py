"""The device graph builder (csrc/plan.hip) without a GPU: the exported symbols, their argument checks against the host planner's
codes for the same mistakes, the empty inputs that launch nothing, and the switch - a CPU batch graph takes the host planner and
`build_direction` whatever `graph.DEVICE_PLAN` says.  tests/test_device_plan_gpu.py holds the kernels to the host path bit for bit."""
import ctypes
import importlib

import torch

import bot_amd
from bot_amd import _C, synth
from bot_amd.sampling import Subgraph

G = importlib.import_module("bot_amd.graph")            # (bot_amd.graph the attribute is dgl.graph's stand-in, a function)

NAMES = ("bot_row_plan_device_workspace_bytes", "bot_row_plan_size_device", "bot_row_plan_fill_device", "bot_csc_transpose_workspace_bytes",
         "bot_csc_transpose_i32")
E_NULL, E_RANGE, E_PLAN = -1, -2, -4
BIG = 2 ** 31 - 1


def _buffers():
    buf = (ctypes.c_int32 * 64)()
    out = (ctypes.c_int64 * 16)()
    return buf, out, ctypes.addressof(buf), ctypes.addressof(out)


def test_symbols_are_exported_and_the_abi_number_stays():
    lib = _C._lib
    for name in NAMES:
        assert name in _C.EXPORTED and hasattr(lib, name)
    assert lib.bot_abi_version() == 19
    assert set(_C.PLAN_COUNTS) == {"device_plan", "device_transpose", "host_plan"}


def test_planner_argument_checks_return_the_host_planners_codes():
    lib = _C._lib
    buf, out, p, o = _buffers()
    big = 1 << 20
    host = lambda indptr, n_rows, chunk: lib.bot_row_plan_size_host(indptr, n_rows, chunk, o, o + 8, o + 16)
    size = lambda indptr, n_rows, chunk, ws=p, sizes=o: lib.bot_row_plan_size_device(indptr, n_rows, chunk, ws, big, sizes, None)
    fill = lambda indptr, n_rows, chunk: lib.bot_row_plan_fill_device(indptr, n_rows, chunk, p, big, n_rows, 0, 0, p, p, p, None)
    for args, code in (((None, 4, 64), E_NULL), ((p, -1, 64), E_RANGE), ((p, BIG, 64), E_RANGE), ((p, 4, 0), E_RANGE), ((p, 4, -3), E_RANGE)):
        assert host(*args) == code                                              # the specification's code for this mistake
        assert size(*args) == code and fill(*args) == code
    assert b"row plan" in lib.bot_last_error()
    # NULL outputs: the host planner's BOT_E_NULL (its own: lib.bot_row_plan_size_host(p, 4, 64, None, ...))
    assert lib.bot_row_plan_size_host(p, 4, 64, None, o, o) == E_NULL
    assert size(p, 4, 64, sizes=None) == E_NULL
    assert size(p, 4, 64, ws=None) == E_NULL                                    # checked before any launch: no GPU is needed
    assert lib.bot_row_plan_fill_device(p, 4, 64, p, big, 4, 0, 0, None, p, p, None) == E_NULL
    assert lib.bot_row_plan_fill_device(p, 4, 64, p, big, 4, 0, 0, p, p, None, None) == E_NULL
    assert lib.bot_row_plan_fill_device(p, 4, 64, None, big, 4, 0, 0, p, p, p, None) == E_NULL
    assert lib.bot_row_plan_fill_device(p, 4, 64, p, big, 5, 1, 2, p, None, p, None) == E_NULL      # long rows, but no long_rows
    # a workspace below bot_row_plan_device_workspace_bytes, the planner's own chunk bound
    need = lib.bot_row_plan_device_workspace_bytes(4)
    assert need > 0 and lib.bot_row_plan_device_workspace_bytes(-1) == -1 and lib.bot_row_plan_device_workspace_bytes(BIG) == -1
    assert lib.bot_row_plan_size_device(p, 4, 64, p, need - 1, o, None) == E_RANGE
    assert size(p, 4, 1025) == E_RANGE and fill(p, 4, 1025) == E_RANGE
    assert _C.DEVICE_PLAN_MAX_CHUNK == 1024 and _C.default_chunk(10 ** 12) <= _C.DEVICE_PLAN_MAX_CHUNK
    # sizes that belong to no plan of 4 rows -> the host planner's BOT_E_PLAN
    for n_items, n_long, n_slots in ((5, 0, 0), (4, 1, 1), (4, 0, 2), (9, 5, 10), (3, -1, 0)):
        assert lib.bot_row_plan_fill_device(p, 4, 64, p, big, n_items, n_long, n_slots, p, p, p, None) == E_PLAN


def test_transpose_argument_checks():
    lib = _C._lib
    buf, out, p, o = _buffers()
    big = 1 << 20
    call = lambda indptr=p, indices=p, n_dst=4, n_src=4, nnz=3, a=p, b=p, c=p, bad=o, ws=p, size=big: \
        lib.bot_csc_transpose_i32(indptr, indices, n_dst, n_src, nnz, a, b, c, bad, ws, size, None)
    for kw in (dict(indptr=None), dict(indices=None), dict(a=None), dict(b=None), dict(c=None), dict(bad=None), dict(ws=None)):
        assert call(**kw) == E_NULL, kw
    for kw in (dict(nnz=-1), dict(nnz=BIG), dict(n_src=-1), dict(n_src=BIG), dict(n_dst=-1), dict(n_dst=BIG), dict(n_src=0), dict(n_dst=0),
               dict(size=lib.bot_csc_transpose_workspace_bytes(3) - 1)):
        assert call(**kw) == E_RANGE, kw
    assert b"csc transpose" in lib.bot_last_error()
    assert lib.bot_csc_transpose_workspace_bytes(-1) == -1 and lib.bot_csc_transpose_workspace_bytes(BIG) == -1


def test_empty_inputs_launch_nothing():
    """No rows / no entries: 0 with nothing launched, so no GPU is needed."""
    lib = _C._lib
    buf, out, p, o = _buffers()
    assert lib.bot_row_plan_size_device(p, 0, 64, None, 0, o, None) == 0
    assert lib.bot_row_plan_fill_device(p, 0, 64, None, 0, 0, 0, 0, None, None, p, None) == 0
    assert lib.bot_csc_transpose_i32(p, None, 4, 4, 0, p, None, None, o, None, 0, None) == 0
    assert lib.bot_csc_transpose_i32(p, None, 0, 0, 0, p, None, None, o, None, 0, None) == 0
    assert lib.bot_row_plan_device_workspace_bytes(0) == 0 and lib.bot_csc_transpose_workspace_bytes(0) == 0


def test_a_cpu_batch_graph_takes_the_host_path_with_the_device_plan_on(monkeypatch):
    n = 300
    rs, rd = synth.powerlaw_edges(n, 2500, 1)
    g = bot_amd.preprocess(bot_amd.Graph(rs, rd, n))
    csc = g.csc
    assert G.DEVICE_PLAN is True and G.device_plan_enabled()
    monkeypatch.setenv("BOT_DEVICE_PLAN", "0")
    assert not G.device_plan_enabled()                                          # read at call time
    monkeypatch.delenv("BOT_DEVICE_PLAN")
    monkeypatch.setattr(G, "DEVICE_PLAN", False)
    assert not G.device_plan_enabled()
    monkeypatch.setattr(G, "DEVICE_PLAN", True)
    before = dict(_C.PLAN_COUNTS)
    # a host-built CSC of the subgraph contract (the whole graph under its own numbering), as the host tests' stand-ins hand over
    sub = Subgraph(g, torch.arange(n, dtype=torch.int32), csc.indptr.long(), csc.indices, csc.eid)
    assert _C.PLAN_COUNTS["host_plan"] == before["host_plan"] + 1
    csr, c2c = sub.csr, sub.csr2csc
    assert _C.PLAN_COUNTS["host_plan"] == before["host_plan"] + 2
    assert _C.PLAN_COUNTS["device_plan"] == before["device_plan"] and _C.PLAN_COUNTS["device_transpose"] == before["device_transpose"]
    s, d = sub.edges()
    want = G.build_direction(s, d, n, g._chunk)                                 # the CSR as any graph's is built from the edge list
    for name in ("indptr", "indices", "eid", "items", "long_rows", "long_ptr"):
        a, b = getattr(csr, name), getattr(want, name)
        assert (a is None and b is None) or torch.equal(a, b), name
    assert torch.equal(sub.csc.items, csc.items) and torch.equal(c2c, csr.eid)  # edge id = CSC position
