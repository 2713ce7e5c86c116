"""The guard harness (tests/guard_ops.py) must see what it claims to see: CPU tensors and a Python stand-in for "the kernel",
one planted defect per case, each reported against the right region.  Nothing here touches a GPU."""
import re

import pytest
import torch

from guard_ops import ALIGN, EDGE, TCFD_EWORKSPACE, Arena, GuardError, Out, nbytes, run_guarded

N = 37                      # float64 elements: 296 bytes, so every region has alignment slack behind it
WS_NEED = 1000              # bytes; 24 bytes of slack up to the next 256-byte boundary


def make_arena():
    return Arena("cpu", [("x", N * 8), ("ws", WS_NEED), ("y", N * 8), ("z", N * 8)], moat=4096)


def stand_in(arena, defect=None):
    """y = 2 x + 1 through a scratch copy of x, z = -x.  ``defect`` plants one fault."""
    def call(ws_bytes):
        if ws_bytes < WS_NEED:
            return TCFD_EWORKSPACE
        x = arena.view("x", torch.float64, (N,))
        tmp = arena.view("ws", torch.float64, (N,))
        y = arena.view("y", torch.float64, (N,))
        z = arena.view("z", torch.float64, (N,))
        tmp.copy_(x)
        y.copy_(2 * tmp + 1)
        z.copy_(-x)
        oy = arena.offset["y"]
        if defect == "past":
            arena.buf[oy + N * 8] = 7
        elif defect == "before":
            arena.buf[oy - 1] = 7
        elif defect == "stride":
            arena.buf[oy + 2 * N * 8 + 5] = 7     # a whole buffer stride beyond y: still inside the moat behind it
        elif defect == "ws_slack":
            arena.buf[arena.offset["ws"] + WS_NEED + 3] = 7
        elif defect == "unwritten":
            y[N - 1] = torch.frombuffer(bytearray([state["byte"]] * 8), dtype=torch.float64)[0]
        elif defect == "input":
            x[4] += 1.0
        elif defect == "ws_read":
            # reads a scratch byte it never wrote (the last one) into the low mantissa byte of y[3]
            arena.raw("y")[3 * 8] = arena.raw("ws")[WS_NEED - 1]
        return 0

    state = {"byte": 0xFF}
    return call, state


def guarded(defect):
    arena = make_arena()
    x = torch.linspace(-1, 1, N, dtype=torch.float64)
    call, state = stand_in(arena, defect)

    def wrapped(ws_bytes):
        # the stand-in for "an element left unwritten" needs the poison value of the current run
        state["byte"] = int(arena.buf[0])
        return call(ws_bytes)

    return run_guarded(wrapped, arena, {"x": x}, {"y": Out(torch.float64, (N,)), "z": Out(torch.float64, (N,))}, "ws",
                       need=WS_NEED, baseline={"y": 2 * x + 1, "z": -x}, last_error=lambda: b"workspace too small",
                       what="stand-in")


def test_layout_is_aligned_and_exact():
    arena = Arena("cpu", [("a", 1), ("b", 255), ("c", 256), ("d", 257), ("e", 0)], moat=1)
    assert arena.buf.data_ptr() % ALIGN == 0
    prev_end = 0
    for name, size in (("a", 1), ("b", 255), ("c", 256), ("d", 257), ("e", 0)):
        assert arena.ptr(name) % ALIGN == 0 and arena.offset[name] % ALIGN == 0
        assert arena.raw(name).numel() == size == arena.size[name]
        assert arena.offset[name] - prev_end >= (EDGE if name == "a" else ALIGN)   # a moat in front of every region
        assert bool(arena.is_moat[prev_end:arena.offset[name]].all())
        assert not bool(arena.is_moat[arena.offset[name]:arena.offset[name] + size].any())
        prev_end = arena.offset[name] + size
    assert arena.total - prev_end >= EDGE and bool(arena.is_moat[prev_end:].all())
    with pytest.raises(AssertionError):
        arena.view("b", torch.float64, (32,))       # 256 bytes do not fit a 255-byte region: the slack is moat


def test_edge_moats_hold_the_largest_region():
    big = EDGE + 12345
    arena = Arena("cpu", [("small", 8), ("big", big)])
    assert arena.offset["small"] >= big and arena.total - (arena.offset["big"] + big) >= big
    assert arena.offset["big"] - (arena.offset["small"] + 8) >= 1 << 20


def test_poison_keeps_inputs_and_moats_report_their_neighbour():
    arena = make_arena()
    arena.view("x", torch.float64, (N,)).fill_(3.0)
    arena.poison(0xFF, keep=["x"])
    assert bool((arena.view("x", torch.float64, (N,)) == 3.0).all())
    assert bool((arena.raw("y") == 0xFF).all()) and bool((arena.raw("ws") == 0xFF).all())
    assert torch.isnan(arena.view("y", torch.float64, (N,))).all() and torch.isnan(arena.view("y", torch.float32, (2 * N,))).all()
    assert arena.moats_intact(0xFF) == (True, "")
    arena.buf[arena.offset["z"] - 2] = 0
    arena.buf[arena.offset["z"] + N * 8] = 0
    ok, msg = arena.moats_intact(0xFF)
    assert not ok and "2 byte(s) before region 'z'" in msg and "1 byte(s) past the end of region 'z'" in msg


def test_clean_stand_in_passes():
    out = guarded(None)
    x = torch.linspace(-1, 1, N, dtype=torch.float64)
    assert torch.equal(out["y"], 2 * x + 1) and torch.equal(out["z"], -x)


@pytest.mark.parametrize("defect, pattern", [
    ("past", r"1 byte\(s\) past the end of region 'y'"),
    ("before", r"1 byte\(s\) before region 'y'"),
    ("stride", r"past the end of region 'y'"),
    ("ws_slack", r"4 byte\(s\) past the end of region 'ws'"),
    ("unwritten", r"output region 'y': 1 element\(s\) not finite .* first at index \(36,\)"),
    ("input", r"read-only input region 'x' was modified \(\d+ bytes, first at \+3[2-9]\)"),
    ("ws_read", r"output region 'y' differs between the 0xFF run and the 0x00 run"),
])
def test_planted_defect_is_reported_against_its_region(defect, pattern):
    with pytest.raises(GuardError) as e:
        guarded(defect)
    assert re.search(pattern, str(e.value)), str(e.value)
    assert str(e.value).startswith("stand-in: ")


def test_unwritten_output_is_seen_through_the_baseline_when_the_poison_is_finite():
    """An element left at 0x00 poison is a finite 0.0: the 0xFF run (NaN) and the comparison across runs catch it."""
    arena = Arena("cpu", [("y", 4 * 4)], moat=256)

    def call(_):
        arena.view("y", torch.float32, (4,))[:3] = 1.0
        return 0

    with pytest.raises(GuardError, match="region 'y'"):
        run_guarded(call, arena, {}, {"y": Out(torch.float32, (4,))})


def test_in_place_alias_and_untouched_elements():
    arena = Arena("cpu", [("x", N * 8), ("y", 6 * 4)], moat=256)
    x = torch.arange(N, dtype=torch.float64)

    def call(_):
        arena.view("x", torch.float64, (N,)).mul_(2)
        y = arena.view("y", torch.float32, (3, 2))
        y[0], y[2] = 1.0, 3.0                        # sample 1 is "out of range": nothing written for it
        return 0

    keep = torch.tensor([False, True, False])
    out = run_guarded(call, arena, {"x": x}, {"x": Out(torch.float64, (N,)), "y": Out(torch.float32, (3, 2), untouched=keep)},
                      baseline={"x": 2 * x})
    assert torch.equal(out["x"], 2 * x)

    def bad(_):
        call(_)
        arena.view("y", torch.float32, (3, 2))[1, 1] = 0.5
        return 0

    with pytest.raises(GuardError, match="region 'y': elements the contract leaves alone were written"):
        run_guarded(bad, arena, {"x": x}, {"x": Out(torch.float64, (N,)), "y": Out(torch.float32, (3, 2), untouched=keep)})


def test_a_result_that_leans_on_the_previous_call_is_seen_on_the_dirty_workspace():
    """Scratch that is accumulated into instead of written: right on 0x00 poison, NaN on 0xFF, and -- were the first poison
    finite -- still caught by the third run, whose workspace holds what the second call left."""
    arena = Arena("cpu", [("x", 8 * 4), ("ws", 8 * 4), ("y", 8 * 4)], moat=256)
    x = torch.arange(8, dtype=torch.int32)

    def call(_):
        tmp = arena.view("ws", torch.int32, (8,))
        tmp += arena.view("x", torch.int32, (8,))            # integers: the 0xFF poison is -1, not a NaN
        arena.view("y", torch.int32, (8,)).copy_(tmp)
        return 0

    with pytest.raises(GuardError, match="region 'y' differs between the 0xFF run and the 0x00 run"):
        run_guarded(call, arena, {"x": x}, {"y": Out(torch.int32, (8,))}, "ws")

    def lucky(_):       # the same defect hidden from both poisons: the scratch is cleared when it holds a poison pattern
        tmp = arena.view("ws", torch.int32, (8,))
        if bool((tmp == -1).all()) or bool((tmp == 0).all()):
            tmp.zero_()
        tmp += arena.view("x", torch.int32, (8,))
        arena.view("y", torch.int32, (8,)).copy_(tmp)
        return 0

    with pytest.raises(GuardError, match="region 'y' differs between the 0xFF run and the run on a dirty workspace"):
        run_guarded(lucky, arena, {"x": x}, {"y": Out(torch.int32, (8,))}, "ws")


def test_short_workspace_must_fail_cleanly():
    arena = make_arena()
    x = torch.ones(N, dtype=torch.float64)
    call, _ = stand_in(arena)
    outs = {"y": Out(torch.float64, (N,)), "z": Out(torch.float64, (N,))}
    with pytest.raises(GuardError, match="returned 0, not TCFD_EWORKSPACE, with 998 of 999"):
        run_guarded(lambda b: call(max(b, WS_NEED)), arena, {"x": x}, outs, "ws", need=999)   # a stand-in that never refuses

    def writes_first(ws_bytes):
        arena.view("z", torch.float64, (N,)).fill_(0.0)
        return call(ws_bytes)

    with pytest.raises(GuardError, match="output region 'z' was touched by a call that returned TCFD_EWORKSPACE"):
        run_guarded(writes_first, arena, {"x": x}, outs, "ws", need=WS_NEED)
    with pytest.raises(GuardError, match="without a message"):
        run_guarded(call, arena, {"x": x}, outs, "ws", need=WS_NEED, last_error=lambda: b"")
    assert nbytes(torch.complex128, (3, 5)) == 240


# ---- coverage of tests/test_memory_contract_gpu.py: every entry point that takes a workspace size has a guarded case
def _workspace_entry_points():
    """The tcfd_* symbols of ``_lib.SIGNATURES`` whose prototype in include/tcfd.h has a ``workspace_bytes`` / ``ws_bytes``
    argument (the signature table holds types only: ``void*, size_t, void* stream`` at the end of the argument list)."""
    import ctypes
    import os

    from torch_cfd_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(_lib.INCLUDE, "tcfd.h")).read(), flags=re.S)    # comments name entry points too
    protos = re.findall(r"\b(tcfd_\w+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S)
    by_name = {name for name, args in protos if re.search(r"size_t\s+(workspace_bytes|ws_bytes)\b", args)}
    tail = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    by_type = {name for name, (_, args) in _lib.SIGNATURES.items() if list(args[-3:]) == tail}
    assert by_name == by_type, (sorted(by_name ^ by_type), "header and signature table disagree")
    return by_name


def test_every_workspace_entry_point_has_a_guarded_case():
    import inspect

    import test_memory_contract_gpu as M
    from torch_cfd_amd import _lib

    takers = _workspace_entry_points()
    assert len(takers) >= 29 and "tcfd_ns2d_step" in takers and "tcfd_h1_sums" in takers
    missing = sorted(takers - set(M.COVERAGE))
    assert not missing, f"entry points that take a workspace but have no guarded case: {missing}"
    sizes = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    assert len(sizes) == 11 and not sizes - set(M.COVERAGE), sorted(sizes - set(M.COVERAGE))    # the twelfth is the irfft2 prefix rule
    for entry, tests in M.COVERAGE.items():
        assert tests, entry
        for name in tests:
            fn = getattr(M, name, None)
            assert callable(fn), f"{entry}: no test {name}"
            if entry.startswith("tcfd_"):
                # the call itself, `<library>.<entry>(`: tcfd_irfft2_subsample( does not stand in for tcfd_irfft2(
                src = inspect.getsource(fn) + inspect.getsource(M.Ns)
                assert re.search(r"\." + re.escape(entry) + r"\(", src), f"{name} does not call {entry}"
