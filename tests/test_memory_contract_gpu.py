"""The memory contract of the C ABI (include/tcfd.h, Conventions), checked with guarded, poisoned buffers.

Every case goes through ``guard_ops.run_guarded``: the call runs on raw pointers into one arena whose regions have exactly
the sizes the header promises suffice, with moats around them; it must return 0, leave moats and read-only inputs alone, write
every output element, give the same bits for 0xFF poison, 0x00 poison and a dirty workspace, the same bits as the Python wrapper
(roomy torch buffers -- the path the oracle and golden tests pin), and with one workspace byte less return TCFD_EWORKSPACE
without touching anything.

COVERAGE below lists entry point against case; tests/test_guard_host.py checks that every symbol of ``_lib.SIGNATURES`` that
takes a workspace size occurs in it, so a later entry point cannot be added without a guarded case.

No TCFD_GRAPH / TCFD_OVERLAP / torch.cuda.graph here: graph replay has its own tests.
"""
import ctypes
import functools
import math

import pytest
import torch

from guard_ops import Arena, Out, nbytes, run_guarded, TCFD_EWORKSPACE

pytestmark = pytest.mark.gpu

# entry point (or size function) -> the tests of this file that run it guarded
COVERAGE = {
    "tcfd_ns2d_workspace_bytes": ["test_ns2d_step", "test_ns2d_explicit", "test_size_functions_document_zero"],
    "tcfd_ns2d_jvp_workspace_bytes": ["test_ns2d_jvp", "test_size_functions_document_zero"],
    "tcfd_ns2d_refine_workspace_bytes": ["test_ns2d_refine", "test_size_functions_document_zero"],
    "field_bytes (irfft2 prefix rule)": ["test_ns2d_transforms"],
    "tcfd_fno_workspace_bytes": ["test_fno_transforms"],
    "tcfd_loss_workspace_bytes": ["test_sobolev_loss"],
    "tcfd_residual_workspace_bytes": ["test_residual_loss"],
    "tcfd_lp_sums_workspace_bytes": ["test_lp_sums"],
    "tcfd_h1_sums_workspace_bytes": ["test_h1_sums"],
    "tcfd_fvm_workspace_bytes": ["test_fvm"],
    "tcfd_fvm_step_vjp_workspace_bytes": ["test_fvm"],
    "tcfd_grf_spectrum_workspace_bytes": ["test_grf_spectrum"],
    "tcfd_ns2d_step": ["test_ns2d_step"],
    "tcfd_ns2d_step_imex": ["test_ns2d_step"],
    "tcfd_ns2d_explicit_terms": ["test_ns2d_explicit"],
    "tcfd_ns2d_explicit_terms_vjp": ["test_ns2d_explicit"],
    "tcfd_ns2d_stream_residual": ["test_ns2d_explicit"],
    "tcfd_ns2d_velocity": ["test_ns2d_explicit"],
    "tcfd_ns2d_explicit_terms_jvp": ["test_ns2d_jvp"],
    "tcfd_ns2d_step_jvp": ["test_ns2d_jvp"],
    "tcfd_rfft2": ["test_ns2d_transforms"],
    "tcfd_irfft2": ["test_ns2d_transforms"],
    "tcfd_irfft2_subsample": ["test_ns2d_transforms"],
    "tcfd_ns2d_refine": ["test_ns2d_refine"],
    "tcfd_ns2d_refine_vjp": ["test_ns2d_refine"],
    "tcfd_ns2d_stage_update": ["test_ns2d_stage_kernels"],
    "tcfd_ns2d_stage_update_vjp": ["test_ns2d_stage_kernels"],
    "tcfd_ns2d_vjp_combine": ["test_ns2d_stage_kernels"],
    "tcfd_fno_spectral_conv": ["test_fno_transforms"],
    "tcfd_fno_forward_trunc": ["test_fno_transforms"],
    "tcfd_fno_forward_trunc_kt": ["test_fno_transforms"],
    "tcfd_fno_inverse_trunc": ["test_fno_transforms", "test_fno_resample"],
    "tcfd_fno_inverse_trunc_acc": ["test_fno_transforms"],
    "tcfd_fno_inverse_trunc_last": ["test_fno_transforms"],
    "tcfd_fno_inverse_trunc_residual": ["test_fno_transforms"],
    "tcfd_fno_inverse_trunc_kt": ["test_fno_transforms"],
    "tcfd_fno_contract": ["test_fno_contract"],
    "tcfd_fno_contract_adjoint": ["test_fno_contract"],
    "tcfd_fno_contract_wgrad": ["test_fno_contract"],
    "tcfd_fno_pointwise": ["test_fno_pointwise"],
    "tcfd_fno_pointwise_pre": ["test_fno_pointwise"],
    "tcfd_fno_pointwise_f64": ["test_fno_pointwise_f64"],
    "tcfd_fno_pointwise_bwd_out": ["test_fno_pointwise"],      # (P = 630 at width 10 only: width 16 has no backward kernel there)
    "tcfd_fno_pointwise_bwd_pe": ["test_fno_pointwise_bwd_pe"],
    "tcfd_sobolev_loss": ["test_sobolev_loss"],
    "tcfd_sobolev_loss_backward": ["test_sobolev_loss"],
    "tcfd_residual_loss": ["test_residual_loss"],
    "tcfd_residual_loss_backward": ["test_residual_loss"],
    "tcfd_lp_sums": ["test_lp_sums"],
    "tcfd_lp_sums_bwd": ["test_lp_sums"],
    "tcfd_h1_sums": ["test_h1_sums"],
    "tcfd_h1_sums_bwd": ["test_h1_sums"],
    "tcfd_weighted_sqnorm": ["test_training_reductions"],
    "tcfd_row_moments": ["test_training_reductions"],
    "tcfd_row_moments_f64": ["test_training_reductions"],
    "tcfd_sum_rows": ["test_training_reductions"],
    "tcfd_sum_t_into_last": ["test_training_reductions"],
    "tcfd_fno_sample_outer_sums": ["test_training_reductions"],
    "tcfd_fvm_explicit_terms": ["test_fvm_schemes"],
    "tcfd_fvm_explicit_terms_vjp": ["test_fvm_schemes"],
    "tcfd_fvm_project": ["test_fvm"],
    "tcfd_fvm_step": ["test_fvm"],
    "tcfd_fvm_step_vjp": ["test_fvm"],
    "tcfd_grf_spectrum": ["test_grf_spectrum"],
    "tcfd_data_window": ["test_data_window"],
    "tcfd_data_fno3d_batch": ["test_data_fno3d_batch"],
    "tcfd_data_affine": ["test_data_affine"],
    "tcfd_data_moments": ["test_data_moments"],
}

L = 2 * math.pi
REAL = {"f32": torch.float32, "f64": torch.float64}
CPLX = {"f32": torch.complex64, "f64": torch.complex128}
CODE = {"f32": 0, "f64": 1}


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _release_plans_and_arenas():
    """The plans, inputs and arenas of this file (a few GB at 1024^2 and 2048^2) do not outlive it."""
    yield
    for cached in (ns, _mcw, _refine_setup, _fvm_setup):
        cached.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _L():
    from torch_cfd_amd import _lib

    return _lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _darr(v):
    from torch_cfd_amd import _lib

    return _lib.darray(v) if v is not None else None


def guard(what, ins, outs, call, need=None, baseline=None, nullable_ws=False):
    """One guarded case.  ``ins``: region -> tensor; ``outs``: region -> Out (a name in both: an allowed alias); ``need``: the
    workspace bytes the size function promised (None / 0: no workspace region); ``call(P, ws_ptr, ws_bytes)``: the ctypes
    call, ``P(name)`` = the arena pointer of a region (None for a name of None)."""
    regions = [(k, nbytes(t.dtype, t.shape)) for k, t in ins.items()]
    if need:
        regions.append(("ws", int(need)))
    regions += [(k, nbytes(o.dtype, o.shape)) for k, o in outs.items() if k not in ins]
    arena = Arena(_dev(), regions)

    def P(name):
        return arena.ptr(name) if name is not None else None

    def run(ws_bytes):
        with torch.cuda.device(_dev()):
            return call(P, arena.ptr("ws") if need else (None if nullable_ws else arena.buf.data_ptr()), ws_bytes)

    return run_guarded(run, arena, ins, outs, "ws" if need else None, need=int(need or 0), baseline=baseline,
                       last_error=_L().tcfd_last_error, what=what)


def smallest_workspace(ins, outs, call, hi):
    """The smallest workspace size a call does not answer with TCFD_EWORKSPACE (bisection; the size check comes before any
    launch, and the probes that pass run inside an arena with ``hi`` bytes of scratch)."""
    regions = [(k, nbytes(t.dtype, t.shape)) for k, t in ins.items()] + [("ws", int(hi))]
    regions += [(k, nbytes(o.dtype, o.shape)) for k, o in outs.items() if k not in ins]
    arena = Arena(_dev(), regions)
    arena.poison(0x00)
    for k, t in ins.items():
        arena.raw(k).copy_(t.to(_dev()).contiguous().view(-1).view(torch.uint8))
    P = lambda name: arena.ptr(name) if name is not None else None
    with torch.cuda.device(_dev()):
        assert call(P, arena.ptr("ws"), int(hi)) == 0, _L().tcfd_last_error()
        assert call(P, arena.ptr("ws"), 0) == TCFD_EWORKSPACE
        lo = 0                                  # fails
        while hi - lo > 1:
            mid = (lo + hi) // 2
            rc = call(P, arena.ptr("ws"), mid)
            assert rc in (0, TCFD_EWORKSPACE), (rc, _L().tcfd_last_error())
            lo, hi = (lo, mid) if rc == 0 else (mid, hi)
    torch.cuda.synchronize()
    ok, msg = arena.moats_intact(0x00)
    assert ok, msg
    return hi


# ================================================================================================ spectral solver
@functools.lru_cache(maxsize=None)
def _mcw(n, seed, tag):
    from oracle import ns2d as O

    return torch.fft.rfft2(O.mcwilliams_vorticity(n, L, 4, seed, REAL[tag]))


def w_hat(n, batch, tag, seed0=0):
    """(batch, n, m) McWilliams half spectra: three seeds, further batch elements are scaled copies (all distinct)."""
    base = [_mcw(n, seed0 + s, tag) for s in range(min(batch, 3))]
    return torch.stack([base[k % 3] * (1 + 0.125 * (k // 3)) for k in range(batch)]).to(_dev())


class Ns:
    """One operator as the package builds it (tables, forcing spectrum, tuning: the wrapper's own plan) and its inputs."""

    def __init__(self, n, tag, batch, pruned):
        import torch_cfd_amd as tc

        torch.set_default_dtype(REAL[tag])
        try:
            grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
            if pruned:
                # (n = 8: wave number 4 is the Nyquist mode, which the 2/3 rule masks -- such a plan cannot be pruned)
                forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4 if n >= 16 else 2)
                self.op = tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, forcing_fn=forcing,
                                                    solver=tc.RK4CrankNicolsonStepper()).to(_dev())
            else:
                self.op = tc.NavierStokes2DSpectral(1e-3, grid, smooth=False, solver=tc.RK4CrankNicolsonStepper()).to(_dev())
            self.imex2 = tc.IMEXStepper(order=2)
            # the plan samples the forcing when it is built: in the operator's precision, like the tables
            self.plan = self.op._plan(torch.zeros(1, n, n // 2 + 1, dtype=CPLX[tag], device=_dev()))
        finally:
            torch.set_default_dtype(torch.float32)
        self.n, self.m, self.tag, self.pruned = n, n // 2 + 1, tag, pruned
        self.cdt, self.rdt = CPLX[tag], REAL[tag]
        self.h = self.plan.handle
        info = self.plan.info()
        if pruned:
            # (the plan stores a forcing as a sparse list when at most 1 / 64 of its entries are non-zero: the 40 entries of the
            #  8 x 5 half spectrum cannot hold one, so the smallest grid runs the pruned plan with the dense forcing table)
            assert info["keep_cols"] > 0 and info["sparse_forcing"] == (1 if n >= 16 else 0), info
        else:
            assert info["keep_cols"] == 0, info
        if batch == "ragged":    # the smallest batch from 7 up whose last chunk is smaller than the others
            batch = next(b for b in range(7, 65) if self.chunk(b) < b and b % self.chunk(b))
        self.batch = batch
        self.w = w_hat(n, batch, tag)
        self.w2 = w_hat(n, batch, tag, seed0=5) * 0.5
        self.shape = (batch, n, self.m)
        self.dt = 1e-3

    def chunk(self, batch):
        c = ctypes.c_long(0)
        assert _L().tcfd_ns2d_plan_chunking(self.h, batch, ctypes.byref(c), None, None) == 0
        return c.value

    def need(self):
        return _L().tcfd_ns2d_workspace_bytes(self.h, self.batch)

    def out(self, lead=()):
        return Out(self.cdt, tuple(lead) + self.shape)


@functools.lru_cache(maxsize=None)
def ns(n, tag, batch, pruned=True):
    return Ns(n, tag, batch, pruned)


NS_PLANS = [(8, "f64", 5, True), (64, "f32", 3, True), (80, "f64", 2, True), (96, "f32", 2, True), (256, "f32", 3, True),
            (512, "f64", 2, True), (1024, "f64", 9, True), (1024, "f64", "ragged", True), (1024, "f32", 2, True),
            (2048, "f32", 2, True), (64, "f32", 3, False), (1024, "f64", "ragged", False)]
NS_IDS = [f"n{n}-{t}-b{b}-{'pruned' if p else 'unpruned'}" for n, t, b, p in NS_PLANS]


def test_ns2d_cover_conditions():
    """Chunked and ragged-chunk batches are what the table says they are (default cache size, no TCFD_CHUNK)."""
    s9, s7 = ns(1024, "f64", 9), ns(1024, "f64", "ragged")
    assert s9.chunk(9) < 9 and s7.chunk(s7.batch) < s7.batch and s7.batch % s7.chunk(s7.batch) != 0
    assert ns(2048, "f32", 2).chunk(2) == 1                       # single-field chunks
    assert ns(1024, "f32", 2).chunk(2) == 2 and ns(512, "f64", 2).chunk(2) == 2
    # balanced chunks: the need is not monotonic in the batch (4 fields per chunk: 8 = 4 + 4 needs more than 9 = 3 + 3 + 3)
    need = [_L().tcfd_ns2d_workspace_bytes(s9.h, b) for b in range(1, 66)]
    drops = [b + 1 for b in range(len(need) - 1) if need[b + 1] < need[b]]          # batches b whose successor needs less
    assert drops, "no batch whose successor needs less scratch: the chunks are no longer balanced (or no longer chunked)"
    assert all(s9.chunk(b) > s9.chunk(b + 1) for b in drops)


def test_size_functions_document_zero():
    """An empty batch needs no scratch (include/tcfd.h, Conventions), and tcfd_grf_spectrum none without normalize."""
    from torch_cfd_amd import fno

    s, lib = ns(64, "f32", 3), _L()
    fvm, loss = _fvm_setup(8, "f32")[1].handle, _loss_plan(16, "f32")
    fplan = fno._plan((16, 16, 10, 2, 12, 4, 4, 3), _dev(), torch.float32).handle
    sizes = {"ns2d": lib.tcfd_ns2d_workspace_bytes(s.h, 0), "jvp": lib.tcfd_ns2d_jvp_workspace_bytes(s.h, 0),
             "refine": lib.tcfd_ns2d_refine_workspace_bytes(s.h, 0, 3), "fno": lib.tcfd_fno_workspace_bytes(fplan, 0, 3, 5),
             "loss": lib.tcfd_loss_workspace_bytes(loss, 0, 10, 2), "residual": lib.tcfd_residual_workspace_bytes(loss, 0, 10, 1),
             "lp": lib.tcfd_lp_sums_workspace_bytes(0, 578, 1), "h1": lib.tcfd_h1_sums_workspace_bytes(0, 3, 67, 45),
             "fvm": lib.tcfd_fvm_workspace_bytes(fvm, 0), "fvm_vjp": lib.tcfd_fvm_step_vjp_workspace_bytes(fvm, 0),
             "grf": lib.tcfd_grf_spectrum_workspace_bytes(0, 64, 1), "grf without normalize": lib.tcfd_grf_spectrum_workspace_bytes(3, 64, 0)}
    assert all(v == 0 for v in sizes.values()), sizes


@pytest.mark.parametrize("n, tag, batch, pruned", NS_PLANS, ids=NS_IDS)
def test_ns2d_step(n, tag, batch, pruned):
    s, lib = ns(n, tag, batch, pruned), _L()
    B, need = s.batch, s.need()
    sc = s.op._schedule(s.op.solver, s.op.solver.params, s.dt)
    beta, gdt, mu = sc["beta"], sc["gdt"], sc["mu"]
    for steps in (1, 3):
        inv = 1 / (steps * s.dt)
        ref = s.plan.step(s.w, beta, gdt, mu, steps, inv, True)
        guard(f"tcfd_ns2d_step steps={steps}", {"w": s.w}, {"out": s.out(), "dwdt": s.out()},
              lambda P, ws, nb: lib.tcfd_ns2d_step(s.h, P("w"), P("out"), P("dwdt"), B, len(beta), _darr(beta), _darr(gdt), _darr(mu),
                                                   steps, inv, ws, nb, _stream()),
              need, {"out": ref[0], "dwdt": ref[1]})
    ref = s.plan.step(s.w, beta, gdt, mu, 2, 1 / (2 * s.dt), False)[0]
    guard("tcfd_ns2d_step in place", {"w": s.w}, {"w": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_step(s.h, P("w"), P("w"), None, B, len(beta), _darr(beta), _darr(gdt), _darr(mu), 2,
                                               1 / (2 * s.dt), ws, nb, _stream()),
          need, {"w": ref})
    # the order-2 schedule: base0 brings the second intermediate state (upad2) into play
    q = s.imex2.stage_schedule(s.imex2.params, s.dt)
    assert q["base0"] is not None and any(q["base0"])
    ints = (ctypes.c_int * len(q["beta"]))(*[int(v) for v in q["base0"]])
    ref = s.plan.step(s.w, q["beta"], q["gdt"], q["mu"], 2, 1 / (2 * s.dt), True, fa=q["fa"], mu_den=q["mu_den"], base0=q["base0"])
    guard("tcfd_ns2d_step_imex order 2", {"w": s.w}, {"out": s.out(), "dwdt": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_step_imex(s.h, P("w"), P("out"), P("dwdt"), B, len(q["beta"]), _darr(q["fa"]),
                                                    _darr(q["beta"]), _darr(q["gdt"]), _darr(q["mu"]), _darr(q["mu_den"]), ints, 2,
                                                    1 / (2 * s.dt), ws, nb, _stream()),
          need, {"out": ref[0], "dwdt": ref[1]})


@pytest.mark.parametrize("n, tag, batch, pruned", NS_PLANS, ids=NS_IDS)
def test_ns2d_explicit(n, tag, batch, pruned):
    s, lib = ns(n, tag, batch, pruned), _L()
    B, need = s.batch, s.need()
    guard("tcfd_ns2d_explicit_terms", {"w": s.w}, {"out": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_explicit_terms(s.h, P("w"), P("out"), B, ws, nb, _stream()),
          need, {"out": s.plan.explicit_terms(s.w)})
    guard("tcfd_ns2d_explicit_terms_vjp", {"w": s.w, "gm": s.w2}, {"x": s.out((4,))},
          lambda P, ws, nb: lib.tcfd_ns2d_explicit_terms_vjp(s.h, P("w"), P("gm"), P("x"), B, ws, nb, _stream()),
          need, {"x": s.plan.explicit_terms_vjp(s.w, s.w2)})
    psi, res = s.plan.stream_residual(s.w, s.w2)
    guard("tcfd_ns2d_stream_residual", {"w": s.w, "wt": s.w2}, {"psi": s.out(), "res": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_stream_residual(s.h, P("w"), P("wt"), P("psi"), P("res"), B, ws, nb, _stream()),
          need, {"psi": psi, "res": res})
    guard("tcfd_ns2d_stream_residual psi=NULL", {"w": s.w, "wt": s.w2}, {"res": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_stream_residual(s.h, P("w"), P("wt"), None, P("res"), B, ws, nb, _stream()),
          need, {"res": res})
    guard("tcfd_ns2d_stream_residual residual=NULL", {"w": s.w, "wt": s.w2}, {"psi": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_stream_residual(s.h, P("w"), P("wt"), P("psi"), None, B, ws, nb, _stream()),
          need, {"psi": psi})
    (uh, vh), psi = s.plan.velocity(s.w)
    guard("tcfd_ns2d_velocity", {"w": s.w}, {"u": s.out(), "v": s.out(), "psi": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_velocity(s.h, P("w"), P("u"), P("v"), P("psi"), B, _stream()),
          None, {"u": uh, "v": vh, "psi": psi})
    guard("tcfd_ns2d_velocity psi=NULL", {"w": s.w}, {"u": s.out(), "v": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_velocity(s.h, P("w"), P("u"), P("v"), None, B, _stream()),
          None, {"u": uh, "v": vh})
    guard("tcfd_ns2d_velocity u=NULL", {"w": s.w}, {"v": s.out(), "psi": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_velocity(s.h, P("w"), None, P("v"), P("psi"), B, _stream()),
          None, {"v": vh, "psi": psi})


JVP_PLANS = [(8, "f64", 5), (64, "f32", 3), (96, "f32", 2), (1024, "f64", 6), (1280, "f64", 2)]


@pytest.mark.parametrize("n, tag, batch", JVP_PLANS, ids=[f"n{n}-{t}-b{b}" for n, t, b in JVP_PLANS])
def test_ns2d_jvp(n, tag, batch):
    s, lib = ns(n, tag, batch), _L()
    B = s.batch
    need = lib.tcfd_ns2d_jvp_workspace_bytes(s.h, B)
    if n == 1024:    # chunked: the scratch stops growing at one chunk (half the fields of a chunk of the plain step)
        assert need < lib.tcfd_ns2d_jvp_workspace_bytes(s.h, 1) * B
    if n == 1280:    # the whole-batch branch: 16 fields of the whole batch, each what tcfd_irfft2 stages (the padded pitch)
        field = smallest_workspace({"w": s.w}, {"out": Out(s.rdt, (B, n, n))},
                                   lambda P, ws, nb: lib.tcfd_irfft2(s.h, P("w"), P("out"), B, ws, nb, _stream()), s.need())
        assert s.chunk(B) == B and need == 16 * field and field >= nbytes(s.cdt, s.shape)
    f, df = s.plan.explicit_terms_jvp(s.w, s.w2)
    guard("tcfd_ns2d_explicit_terms_jvp", {"w": s.w, "dw": s.w2}, {"f": s.out(), "df": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_explicit_terms_jvp(s.h, P("w"), P("dw"), P("f"), P("df"), B, ws, nb, _stream()),
          need, {"f": f, "df": df})
    guard("tcfd_ns2d_explicit_terms_jvp out_f=NULL", {"w": s.w, "dw": s.w2}, {"df": s.out()},
          lambda P, ws, nb: lib.tcfd_ns2d_explicit_terms_jvp(s.h, P("w"), P("dw"), None, P("df"), B, ws, nb, _stream()),
          need, {"df": df})
    sc = s.op._schedule(s.op.solver, s.op.solver.params, s.dt)
    beta, gdt, mu = sc["beta"], sc["gdt"], sc["mu"]
    o, do = s.plan.step_jvp(s.w, s.w2, beta, gdt, mu, 2)

    def step(P, wo, dwo, ws, nb):
        return lib.tcfd_ns2d_step_jvp(s.h, P("w"), P("dw"), P(wo), P(dwo), B, len(beta), None, _darr(beta), _darr(gdt), _darr(mu),
                                      None, None, 2, ws, nb, _stream())

    guard("tcfd_ns2d_step_jvp", {"w": s.w, "dw": s.w2}, {"out": s.out(), "dout": s.out()},
          lambda P, ws, nb: step(P, "out", "dout", ws, nb), need, {"out": o, "dout": do})
    guard("tcfd_ns2d_step_jvp in place", {"w": s.w, "dw": s.w2}, {"w": s.out(), "dw": s.out()},
          lambda P, ws, nb: step(P, "w", "dw", ws, nb), need, {"w": o, "dw": do})


TRANSFORM_PLANS = [p for p in NS_PLANS if p[3]]


@pytest.mark.parametrize("n, tag, batch, pruned", TRANSFORM_PLANS, ids=NS_IDS[:len(TRANSFORM_PLANS)])
def test_ns2d_transforms(n, tag, batch, pruned):
    s, lib = ns(n, tag, batch, pruned), _L()
    B = s.batch
    x = s.plan.irfft2(s.w)
    real = Out(s.rdt, (B, n, n))
    guard("tcfd_rfft2", {"x": x}, {"out": s.out()},
          lambda P, ws, nb: lib.tcfd_rfft2(s.h, P("x"), P("out"), B, _stream()), None, {"out": s.plan.rfft2(x)})
    # the irfft2 prefix rule: one field of the whole batch in the padded pitch -- found as the size whose predecessor fails
    irfft2 = lambda P, ws, nb: lib.tcfd_irfft2(s.h, P("w"), P("out"), B, ws, nb, _stream())
    field = smallest_workspace({"w": s.w}, {"out": real}, irfft2, s.need())
    assert field % 256 == 0 and field >= nbytes(s.cdt, s.shape) and s.need() >= field
    guard("tcfd_irfft2", {"w": s.w}, {"out": real}, irfft2, field, {"out": x})
    top = lib.tcfd_irfft2_subsample_max_factor(s.h)
    if top < 2:     # n = 8: no one-pass form -- the call says so before it touches anything, and the host runs the two calls
        assert n == 8
        small = torch.full((B, n // 2, n // 2), 7.0, dtype=s.rdt, device=_dev())
        ws = s.plan.workspace(B)
        with torch.cuda.device(_dev()):
            rc = lib.tcfd_irfft2_subsample(s.h, s.w.data_ptr(), small.data_ptr(), B, 2, ws.data_ptr(), ws.numel(), _stream())
        torch.cuda.synchronize()
        assert rc == -1 and lib.tcfd_last_error() and bool((small == 7.0).all())
    for factor in sorted({2, top} if top >= 2 else ()):
        ns_ = n // factor
        guard(f"tcfd_irfft2_subsample factor={factor}", {"w": s.w}, {"out": Out(s.rdt, (B, ns_, ns_))},
              lambda P, ws, nb: lib.tcfd_irfft2_subsample(s.h, P("w"), P("out"), B, factor, ws, nb, _stream()),
              field, {"out": s.plan.irfft2_subsample(s.w, factor)})


REFINE_CASES = [(64, 3, 2, "f64"), (256, 5, 1, "f32")]


@functools.lru_cache(maxsize=None)
def _refine_setup(n, nt, batch, tag):
    import finetune_ops as F
    from torch_cfd_amd.finetune import _refine_plan

    real = REAL[tag]
    kx, ky, lap, mask = F.tables(n, 1.0, batch, True, dtype=real)
    plan = _refine_plan(kx, ky, lap, mask, n, CPLX[tag], _dev())
    w = F.smooth_trajectory(batch, n, nt, real).to(_dev())
    f_hat = plan.rfft2(F.smooth_forcing(batch, n, real).to(_dev()))
    g = [F.smooth_trajectory(batch, n, nt, real, phase=0.4 + k).to(_dev()) for k in range(3)]
    return plan, (kx, ky, lap, mask), w, f_hat, g


@pytest.mark.parametrize("n, nt, batch, tag", REFINE_CASES, ids=[f"n{c[0]}-nt{c[1]}-b{c[2]}-{c[3]}" for c in REFINE_CASES])
@pytest.mark.parametrize("forced", [True, False], ids=["f_hat", "no_f"])
def test_ns2d_refine(n, nt, batch, tag, forced):
    plan, _tables, w, f_hat, g = _refine_setup(n, nt, batch, tag)
    lib, h = _L(), plan.hp.handle
    need = lib.tcfd_ns2d_refine_workspace_bytes(h, batch, nt)
    dt, visc, wgt = 1e-3, 1e-3, (0.25, 0.75)
    fh = f_hat if forced else None
    ins = {"w": w, **({"f": fh} if forced else {})}
    o = Out(w.dtype, tuple(w.shape))
    ref = dict(zip(("ow", "owt", "ores"), plan.refine(w, fh, dt, visc, wgt)))
    for drop in (None, "ow", "owt", "ores"):
        outs = {k: o for k in ("ow", "owt", "ores") if k != drop}
        name = lambda P, k: P(k) if k != drop else None
        guard(f"tcfd_ns2d_refine without {drop}", ins, outs,
              lambda P, ws, nb: lib.tcfd_ns2d_refine(h, P("w"), P("f") if forced else None, name(P, "ow"), name(P, "owt"),
                                                     name(P, "ores"), batch, nt, dt, visc, wgt[0], wgt[1], ws, nb, _stream()),
              need, {k: ref[k] for k in outs})
    for drop in (None, "g0", "g1", "g2", "gf"):
        grads = [None if drop == f"g{k}" else g[k] for k in range(3)]
        want_f = forced and drop != "gf"
        if drop == "gf" and not forced:
            continue
        gw, gf = plan.refine_vjp(w, fh, grads, want_f, dt, visc, wgt)
        gins = {**ins, **{f"g{k}": g[k] for k in range(3) if grads[k] is not None}}
        outs = {"gw": o, **({"gf": Out(f_hat.dtype, tuple(f_hat.shape))} if want_f else {})}
        gp = lambda P, k: P(f"g{k}") if grads[k] is not None else None
        guard(f"tcfd_ns2d_refine_vjp without {drop}", gins, outs,
              lambda P, ws, nb: lib.tcfd_ns2d_refine_vjp(h, P("w"), P("f") if forced else None, gp(P, 0), gp(P, 1), gp(P, 2), P("gw"),
                                                         P("gf") if want_f else None, batch, nt, dt, visc, wgt[0], wgt[1], ws, nb,
                                                         _stream()),
              need, {"gw": gw, **({"gf": gf} if want_f else {})})


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("rows, cols", [(16, 9), (80, 41)])
def test_ns2d_stage_kernels(rows, cols, tag):
    from torch_cfd_amd.autograd import StageUpdate

    lib, B, plane = _L(), 3, rows * cols
    gen = torch.Generator().manual_seed(rows)
    mk = lambda *shape: torch.randn(*shape, dtype=CPLX[tag], generator=gen).to(_dev())
    f, hp, b, g_u, g_h = (mk(B, plane) for _ in range(5))
    lin = (-torch.rand(plane, dtype=REAL[tag], generator=gen)).to(_dev())
    coef = (0.75, -0.5, 1e-3, 2e-4, 3e-4)
    c = (ctypes.c_double * 5)(*coef)
    o = Out(CPLX[tag], (B, plane))
    for prev in (True, False):
        h_ref, u_ref = torch.empty_like(f), torch.empty_like(f)
        StageUpdate._launch("tcfd_ns2d_stage_update", (f, hp if prev else None, b), lin, coef, (h_ref, u_ref), f)
        guard(f"tcfd_ns2d_stage_update h_prev={prev}", {"f": f, "b": b, "lin": lin, **({"hp": hp} if prev else {})},
              {"h": o, "u": o},
              lambda P, ws, nb: lib.tcfd_ns2d_stage_update(P("f"), P("hp") if prev else None, P("b"), P("lin"), c, P("h"), P("u"), B,
                                                           plane, CODE[tag], _stream()),
              None, {"h": h_ref, "u": u_ref})
    for has_gh, want_hp in ((True, True), (False, True), (True, False)):
        refs = {k: torch.empty_like(f) for k in ("g_f", "g_b", *(("g_hp",) if want_hp else ()))}
        StageUpdate._launch("tcfd_ns2d_stage_update_vjp", (g_u, g_h if has_gh else None), lin, coef,
                            (refs["g_f"], refs.get("g_hp"), refs["g_b"]), g_u)
        guard(f"tcfd_ns2d_stage_update_vjp g_h={has_gh} g_hprev={want_hp}",
              {"g_u": g_u, "lin": lin, **({"g_h": g_h} if has_gh else {})}, {k: o for k in refs},
              lambda P, ws, nb: lib.tcfd_ns2d_stage_update_vjp(P("g_u"), P("g_h") if has_gh else None, P("lin"), c, P("g_f"),
                                                               P("g_hp") if want_hp else None, P("g_b"), B, plane, CODE[tag],
                                                               _stream()),
              None, refs)
    X, post = mk(4, B, plane), mk(4, plane)
    ref = torch.empty_like(f)
    with torch.cuda.device(_dev()):      # the wrapper (autograd.FusedExplicitTerms.backward) makes this very call on torch buffers
        assert lib.tcfd_ns2d_vjp_combine(X.data_ptr(), post.data_ptr(), ref.data_ptr(), B, plane, CODE[tag], _stream()) == 0
    guard("tcfd_ns2d_vjp_combine", {"X": X, "post": post}, {"out": o},
          lambda P, ws, nb: lib.tcfd_ns2d_vjp_combine(P("X"), P("post"), P("out"), B, plane, CODE[tag], _stream()), None, {"out": ref})


def roomy(ins, outs, call, need=0):
    """The same call the way every wrapper of the package makes it -- each buffer a torch allocation of its own, the workspace
    larger than asked and its full length passed -- for the entry points whose wrapper is an inline call inside an autograd node."""
    bufs = {k: t.to(_dev()).contiguous().clone() for k, t in ins.items()}
    for k, o in outs.items():
        if k not in bufs:
            bufs[k] = torch.empty(o.shape, dtype=o.dtype, device=_dev())
    ws = torch.empty(2 * int(need) + 4096, dtype=torch.uint8, device=_dev())
    with torch.cuda.device(_dev()):
        rc = call(lambda name: bufs[name].data_ptr() if name is not None else None, ws.data_ptr(), ws.numel())
    assert rc == 0, _L().tcfd_last_error()
    torch.cuda.synchronize()
    return {k: bufs[k] for k in outs}


# ================================================================================================ finite volume
@functools.lru_cache(maxsize=None)
def _fvm_setup(n, tag, scheme="van_leer"):
    import fvm_ops as F
    import fvm_schemes_ops as S
    import torch_cfd_amd as tc
    from torch_cfd_amd import initial_conditions as ic

    torch.set_default_dtype(torch.float64)
    try:
        ph = S.Physics(scheme, n)
        solver = tc.RKStepper(tableau=F.TABLEAUX["ssprk3"], dtype=torch.float64)
        eq = ph.equation(solver)
        ux, uy = ic.filtered_velocity_field(ph.grid(), 2.0, 3.0, random_state=0, device=_dev(), batch_seeds=[0, 1, 2])
        gx, gy = ic.filtered_velocity_field(ph.grid(), 1.0, 2.0, random_state=7, device=_dev(), batch_seeds=[3, 4, 5])
    finally:
        torch.set_default_dtype(torch.float32)
    real = REAL[tag]
    cast = lambda t: t.detach().to(real).contiguous()
    dt = 0.25 * ph.h
    a, b = solver.weights(dt)
    assert len(b) == 3
    return eq, eq._plan(real, _dev()), cast(ux), cast(uy), cast(gx), cast(gy), dt, a, b


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("scheme", ["van_leer", "upwind", "linear", "lax_wendroff"])
def test_fvm_schemes(scheme, tag):
    n, B, lib = 8, 3, _L()
    _eq, plan, ux, uy, gx, gy, dt, _a, _b = _fvm_setup(n, tag, scheme)
    o = Out(REAL[tag], (B, n, n))
    kx, ky = plan.explicit_terms(ux, uy, dt)
    guard(f"tcfd_fvm_explicit_terms {scheme}", {"ux": ux, "uy": uy}, {"kx": o, "ky": o},
          lambda P, ws, nb: lib.tcfd_fvm_explicit_terms(plan.handle, P("ux"), P("uy"), P("kx"), P("ky"), B, dt, _stream()),
          None, {"kx": kx, "ky": ky})
    ox, oy = plan.explicit_terms_vjp(ux, uy, gx, gy, dt)
    guard(f"tcfd_fvm_explicit_terms_vjp {scheme}", {"ux": ux, "uy": uy, "gx": gx, "gy": gy}, {"ox": o, "oy": o},
          lambda P, ws, nb: lib.tcfd_fvm_explicit_terms_vjp(plan.handle, P("ux"), P("uy"), P("gx"), P("gy"), P("ox"), P("oy"), B, dt,
                                                            _stream()),
          None, {"ox": ox, "oy": oy})


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("n", [8, 64, 80])
def test_fvm(n, tag):
    B, lib = 3, _L()
    _eq, plan, ux, uy, gx, gy, dt, a, b = _fvm_setup(n, tag)
    h = plan.handle
    o = Out(REAL[tag], (B, n, n))
    need = lib.tcfd_fvm_workspace_bytes(h, B)
    if n != 8:     # (n = 8 runs all four schemes in test_fvm_schemes)
        kx, ky = plan.explicit_terms(ux, uy, dt)
        guard("tcfd_fvm_explicit_terms", {"ux": ux, "uy": uy}, {"kx": o, "ky": o},
              lambda P, ws, nb: lib.tcfd_fvm_explicit_terms(h, P("ux"), P("uy"), P("kx"), P("ky"), B, dt, _stream()),
              None, {"kx": kx, "ky": ky})
        vx, vy = plan.explicit_terms_vjp(ux, uy, gx, gy, dt)
        guard("tcfd_fvm_explicit_terms_vjp", {"ux": ux, "uy": uy, "gx": gx, "gy": gy}, {"ox": o, "oy": o},
              lambda P, ws, nb: lib.tcfd_fvm_explicit_terms_vjp(h, P("ux"), P("uy"), P("gx"), P("gy"), P("ox"), P("oy"), B, dt, _stream()),
              None, {"ox": vx, "oy": vy})
    # project: "needs a prefix of" the step's workspace -- the smallest size it does not refuse
    px, py = plan.project(ux, uy)
    project = lambda P, ws, nb: lib.tcfd_fvm_project(h, P("ux"), P("uy"), P("ox"), P("oy"), B, ws, nb, _stream())
    prefix = smallest_workspace({"ux": ux, "uy": uy}, {"ox": o, "oy": o}, project, need)
    assert 0 < prefix <= need
    guard("tcfd_fvm_project", {"ux": ux, "uy": uy}, {"ox": o, "oy": o}, project, prefix, {"ox": px, "oy": py})
    guard("tcfd_fvm_project in place", {"ux": ux, "uy": uy}, {"ux": o, "uy": o},
          lambda P, ws, nb: lib.tcfd_fvm_project(h, P("ux"), P("uy"), P("ux"), P("uy"), B, ws, nb, _stream()),
          prefix, {"ux": px, "uy": py})
    sx, sy = plan.step(ux, uy, dt, a, b, 2)
    ca, cb = _darr(a), _darr(b)
    guard("tcfd_fvm_step", {"ux": ux, "uy": uy}, {"ox": o, "oy": o},
          lambda P, ws, nb: lib.tcfd_fvm_step(h, P("ux"), P("uy"), P("ox"), P("oy"), B, 2, 3, ca, cb, dt, ws, nb, _stream()),
          need, {"ox": sx, "oy": sy})
    guard("tcfd_fvm_step in place", {"ux": ux, "uy": uy}, {"ux": o, "uy": o},
          lambda P, ws, nb: lib.tcfd_fvm_step(h, P("ux"), P("uy"), P("ux"), P("uy"), B, 2, 3, ca, cb, dt, ws, nb, _stream()),
          need, {"ux": sx, "uy": sy})
    saved, _, _ = plan.step_saving(ux, uy, dt, a, b, 2)
    bx, by = plan.step_vjp(saved, gx, gy, dt, a, b)
    vneed = lib.tcfd_fvm_step_vjp_workspace_bytes(h, B)
    guard("tcfd_fvm_step_vjp", {"saved": saved, "gx": gx, "gy": gy}, {"ox": o, "oy": o},
          lambda P, ws, nb: lib.tcfd_fvm_step_vjp(h, P("saved"), P("gx"), P("gy"), P("ox"), P("oy"), B, 2, 3, ca, cb, dt, ws, nb,
                                                  _stream()),
          vneed, {"ox": bx, "oy": by})
    guard("tcfd_fvm_step_vjp out == g", {"saved": saved, "gx": gx, "gy": gy}, {"gx": o, "gy": o},
          lambda P, ws, nb: lib.tcfd_fvm_step_vjp(h, P("saved"), P("gx"), P("gy"), P("gx"), P("gy"), B, 2, 3, ca, cb, dt, ws, nb,
                                                  _stream()),
          vneed, {"gx": bx, "gy": by})


# ================================================================================================ losses
def _loss_plan(n, tag):
    from torch_cfd_amd import losses

    key = (n, CODE[tag], _dev())
    if key not in losses._LOSS_PLANS:
        handle = ctypes.c_void_p()
        with torch.cuda.device(_dev()):
            assert _L().tcfd_loss_plan_create(ctypes.byref(handle), n, CODE[tag]) == 0
        losses._LOSS_PLANS[key] = handle
    return losses._LOSS_PLANS[key]


@pytest.mark.parametrize("nfields", [1, 2])
@pytest.mark.parametrize("n, nt, tag", [(16, 10, "f32"), (80, 6, "f64")])
def test_sobolev_loss(n, nt, tag, nfields):
    import losses_ops as LO
    from torch_cfd_amd import losses

    lib, B, real = _L(), 2, REAL[tag]
    x, y = (t.to(_dev()) for t in LO.small_inputs((B, n, n, nt), 21, dtype=real))
    module = losses.SobolevLoss(n_grid=n, relative=(nfields == 2)).to(_dev())
    plan = _loss_plan(n, tag)
    assert lib.tcfd_sobolev_loss_supported(plan, nt, nfields)
    w2 = module._half_spectrum_weights(_dev(), real)
    wf = module._w2_cache[2]
    flags = (nfields, int(nfields == 2), 2, 1, 1)       # as SobolevLoss._fused forms them under a float32 default dtype
    need = lib.tcfd_loss_workspace_bytes(plan, B, nt, nfields)
    sums_ref = torch.empty(nfields * B * nt, dtype=torch.float64, device=_dev())
    out_ref = losses._fused_forward(plan, x, y, w2, losses._loss_workspace(_dev(), need), flags, sums_ref)
    torch.cuda.synchronize()
    assert torch.equal(out_ref, module(x, y))            # ... and that is the module's own path
    ins = {"x": x, "y": y, "w2": w2}
    fwd = lambda P, ws, nb, sums: lib.tcfd_sobolev_loss(plan, P("x"), P("y"), P("w2"), B, nt, nfields, *flags[1:], P("out"), P(sums),
                                                        ws, nb, _stream())
    got = guard("tcfd_sobolev_loss", ins, {"out": Out(real, (1,)), "sums": Out(torch.float64, (nfields * B * nt,))},
                lambda P, ws, nb: fwd(P, ws, nb, "sums"), need, {"out": out_ref.reshape(1), "sums": sums_ref})
    guard("tcfd_sobolev_loss sums=NULL", ins, {"out": Out(real, (1,))}, lambda P, ws, nb: fwd(P, ws, nb, None), need,
          {"out": out_ref.reshape(1)})
    xg = x.clone().requires_grad_(True)
    module(xg, y).backward()
    gout = torch.ones(1, dtype=real, device=_dev())
    bneed = lib.tcfd_loss_workspace_bytes(plan, B, nt, 1)    # "the workspace of a one-field forward call suffices"
    guard("tcfd_sobolev_loss_backward", {"x": x, "y": y, "wf": wf, "sums": got["sums"], "gout": gout},
          {"grad": Out(real, (B, n, n, nt))},
          lambda P, ws, nb: lib.tcfd_sobolev_loss_backward(plan, P("x"), P("y"), P("wf"), P("sums"), P("gout"), B, nt, nfields,
                                                           *flags[1:], P("grad"), ws, nb, _stream()),
          bneed, {"grad": xg.grad})


@pytest.mark.parametrize("b, n, nt", [(2, 16, 1), (3, 16, 10), (2, 80, 6), (2, 96, 4)])
def test_residual_loss(b, n, nt):
    import losses_ops as LO
    from torch_cfd_amd import losses

    tag = "f64" if n == 80 else "f32"
    lib, real = _L(), REAL[tag]
    torch.set_default_dtype(real)
    try:
        module = losses.ResidualLoss(visc=LO.residual_visc(n), n_grid=n, n_t=nt, delta_t=LO.RESIDUAL_DELTA_T)
    finally:
        torch.set_default_dtype(torch.float32)
    w, f, _ = (t.to(_dev()) for t in LO.residual_inputs(b, n, nt, real))
    plan = _loss_plan(n, tag)
    assert lib.tcfd_residual_loss_supported(plan, nt)
    tabs = module._tables(_dev(), real)
    scale, visc = module._scale(b), float(module.visc)
    out_ref, rows_ref = module._launch_forward(plan, w, f, tabs, scale)
    tins = dict(zip(("m2pi", "lap", "ckt", "twt"), tabs))
    need = lib.tcfd_residual_workspace_bytes(plan, b, nt, 0)
    guard("tcfd_residual_loss", {"w": w, "f": f, **tins}, {"out": Out(real, (1,)), "rows": Out(torch.float64, (b * n,))},
          lambda P, ws, nb: lib.tcfd_residual_loss(plan, P("w"), P("f"), P("m2pi"), P("lap"), P("ckt"), P("twt"), visc, scale, b, nt,
                                                   P("out"), P("rows"), ws, nb, _stream()),
          need, {"out": out_ref.reshape(1), "rows": rows_ref})
    out0, rows0 = module._launch_forward(plan, w, None, tabs, scale)
    guard("tcfd_residual_loss f=NULL", {"w": w, **tins}, {"out": Out(real, (1,)), "rows": Out(torch.float64, (b * n,))},
          lambda P, ws, nb: lib.tcfd_residual_loss(plan, P("w"), None, P("m2pi"), P("lap"), P("ckt"), P("twt"), visc, scale, b, nt,
                                                   P("out"), P("rows"), ws, nb, _stream()),
          need, {"out": out0.reshape(1), "rows": rows0})
    bneed = lib.tcfd_residual_workspace_bytes(plan, b, nt, 1)
    gout = torch.ones(1, dtype=real, device=_dev())
    o = Out(real, (b, n, n, nt))
    for want_w, want_f in ((True, True), (True, False), (False, True)):
        wg, fg = w.clone().requires_grad_(want_w), f.clone().requires_grad_(want_f)
        losses._ResidualFn.apply(wg, fg, module, plan, tabs, scale).backward()
        outs = {**({"gw": o} if want_w else {}), **({"gf": o} if want_f else {})}
        ref = {**({"gw": wg.grad} if want_w else {}), **({"gf": fg.grad} if want_f else {})}
        guard(f"tcfd_residual_loss_backward grad_w={want_w} grad_f={want_f}", {"w": w, "f": f, **tins, "rows": rows_ref, "gout": gout},
              outs,
              lambda P, ws, nb: lib.tcfd_residual_loss_backward(plan, P("w"), P("f"), P("m2pi"), P("lap"), P("ckt"), P("twt"), visc,
                                                                scale, P("rows"), P("gout"), b, nt, P("gw") if want_w else None,
                                                                P("gf") if want_f else None, ws, nb, _stream()),
              bneed, ref)


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("outer, reduce, inner", [(3, 578, 1), (2, 70001, 3)])
def test_lp_sums(outer, reduce, inner, tag):
    import losses_ops as LO
    from torch_cfd_amd import losses

    lib, real = _L(), REAL[tag]
    x, y = (t.to(_dev()) for t in LO.small_inputs((outer, reduce, inner), 31, dtype=real))
    need = lib.tcfd_lp_sums_workspace_bytes(outer, reduce, inner)
    if reduce > 578:    # several stage-one workgroups: their partial sums live in the workspace
        assert need > lib.tcfd_lp_sums_workspace_bytes(outer, 578, inner)
    so = Out(torch.float64, (outer, inner))
    cd, cy = (t.to(_dev()) for t in LO.small_inputs((outer, inner), 32, dtype=torch.float64))
    for p in (2.0, 3.0):
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        sd, sy = losses.hip_lp_sums(xg, yg, outer, reduce, inner, p, want_y=True)
        guard(f"tcfd_lp_sums p={p}", {"x": x, "y": y}, {"sd": so, "sy": so},
              lambda P, ws, nb: lib.tcfd_lp_sums(P("x"), P("y"), P("sd"), P("sy"), outer, reduce, inner, p, CODE[tag], ws, nb, _stream()),
              need, {"sd": sd.detach(), "sy": sy.detach()})
        guard(f"tcfd_lp_sums p={p} sum_y=NULL", {"x": x, "y": y}, {"sd": so},
              lambda P, ws, nb: lib.tcfd_lp_sums(P("x"), P("y"), P("sd"), None, outer, reduce, inner, p, CODE[tag], ws, nb, _stream()),
              need, {"sd": sd.detach()})
        ((sd * cd).sum() + (sy * cy).sum()).backward()
        g = Out(real, (outer, reduce, inner))
        guard(f"tcfd_lp_sums_bwd p={p}", {"x": x, "y": y, "cd": cd, "cy": cy}, {"gx": g, "gy": g},
              lambda P, ws, nb: lib.tcfd_lp_sums_bwd(P("x"), P("y"), P("cd"), P("cy"), P("gx"), P("gy"), outer, reduce, inner, p,
                                                     CODE[tag], _stream()),
              None, {"gx": xg.grad, "gy": yg.grad})


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("kmode", [0, 1, 2])
def test_h1_sums(kmode, tag):
    import losses_ops as LO
    from torch_cfd_amd import losses

    lib, real = _L(), REAL[tag]
    N, C, n1, n2, h = 2, 3, 67, 45, 1 / 64
    (preds,) = LO.small_inputs((N, C, n1, n2), 41, 1, dtype=real)
    (tg,) = LO.small_inputs((N, 2 * C, n1, n2), 42, 1, dtype=real)
    (kraw,) = LO.small_inputs((N, 1, n1, n2), 43, 1, dtype=real)
    K = None if kmode == 0 else (torch.tensor([0.7], dtype=real) if kmode == 1 else kraw.abs() + 0.5)
    preds, tg = preds.to(_dev()), tg.to(_dev())
    K = K.to(_dev()) if K is not None else None
    pg = preds.clone().requires_grad_(True)
    s1, s2 = losses._H1SumsFn.apply(pg, tg, K, kmode, h)
    (cot,) = LO.small_inputs((N,), 44, 1, dtype=torch.float64)
    cot = cot.to(_dev())
    (s1 * cot).sum().backward()
    need = lib.tcfd_h1_sums_workspace_bytes(N, C, n1, n2)
    ins = {"p": preds, "t": tg, **({"k": K} if kmode else {})}
    so = Out(torch.float64, (N,))
    guard(f"tcfd_h1_sums kmode={kmode}", ins, {"s1": so, "s2": so},
          lambda P, ws, nb: lib.tcfd_h1_sums(P("p"), P("t"), P("k") if kmode else None, kmode, P("s1"), P("s2"), N, C, n1, n2, h,
                                             CODE[tag], ws, nb, _stream()),
          need, {"s1": s1.detach(), "s2": s2.detach()})
    guard(f"tcfd_h1_sums_bwd kmode={kmode}", {**ins, "cot": cot}, {"grad": Out(real, (N, C, n1, n2))},
          lambda P, ws, nb: lib.tcfd_h1_sums_bwd(P("p"), P("t"), P("k") if kmode else None, kmode, P("cot"), P("grad"), N, C, n1, n2, h,
                                                 CODE[tag], _stream()),
          None, {"grad": pg.grad})


def test_training_reductions():
    """The small reductions at the ragged shapes of tests/test_training_kernels_gpu.py.  Their wrappers are inline calls inside
    autograd nodes (fno.py, losses.py), so the baseline is the same call on torch buffers of its own (``roomy``)."""
    lib = _L()
    gen = torch.Generator().manual_seed(5)

    def both(what, ins, outs, call):
        guard(what, ins, outs, call, None, roomy(ins, outs, call))

    for rows, cols in ((37, 5), (4100, 33), (1, 300)):
        m = torch.randn(rows, cols, generator=gen)
        slices = lib.tcfd_sum_rows_slices(rows)
        both(f"tcfd_sum_rows {rows}x{cols}", {"in": m}, {"out": Out(torch.float64, (cols,)), "scratch": Out(torch.float64, (slices * cols,))},
             lambda P, ws, nb: lib.tcfd_sum_rows(P("in"), P("out"), P("scratch"), rows, cols, _stream()))
    for rows, T, sT in ((1000, 10, 10), (77, 7, 3), (64, 4, 1)):
        d = torch.randn(rows, T, generator=gen)
        both(f"tcfd_sum_t_into_last {rows}x{T}->{sT}", {"d": d}, {"g": Out(torch.float32, (rows, sT))},
             lambda P, ws, nb: lib.tcfd_sum_t_into_last(P("d"), P("g"), rows, T, sT, _stream()))
    for tag in ("f32", "f64"):
        rows, Lr = 3, 16 * 41 * 7 + 5
        x = torch.randn(rows, Lr, generator=gen, dtype=REAL[tag])
        both(f"tcfd_row_moments {tag}", {"x": x}, {"stats": Out(torch.float64, (rows, 2))},
             lambda P, ws, nb: (lib.tcfd_row_moments(P("x"), P("stats"), rows, Lr, _stream()) if tag == "f32" else
                                lib.tcfd_row_moments_f64(P("x"), P("stats"), rows, Lr, _stream())))
        batch, n, m = 3, 80, 41
        z = torch.randn(batch, n * m, generator=gen, dtype=CPLX[tag])
        w2 = torch.rand(n * m, generator=gen, dtype=REAL[tag])
        blocks = max(1, min(64, (n * m + 4095) // 4096))        # as losses.hip_weighted_sqnorm cuts the field
        both(f"tcfd_weighted_sqnorm {tag}", {"z": z, "w2": w2}, {"partial": Out(torch.float64, (batch, blocks))},
             lambda P, ws, nb: lib.tcfd_weighted_sqnorm(P("z"), P("w2"), P("partial"), batch, n * m, blocks, CODE[tag], _stream()))
    b, Pn, wps = 3, 16 * 41, 8
    for C, co, table in ((7, 5, False), (31, 17, True), (40, 9, False)):
        R16, C16 = 16 * ((co + 15) // 16), 16 * ((C + 16) // 16)
        dy = torch.randn(b, co, Pn, generator=gen)
        ins = {"dy": dy, "x": torch.randn(*((b, Pn) if table else (b, C, Pn)), generator=gen)}
        if table:
            ins["pe"] = torch.randn(C, Pn, generator=gen)
        both(f"tcfd_fno_sample_outer_sums C={C} co={co} table={table}", ins, {"tiles": Out(torch.float32, (wps, b, R16 * C16))},
             lambda P, ws, nb: lib.tcfd_fno_sample_outer_sums(P("dy"), P("x"), P("pe") if table else None, P("tiles"), b, C, co, Pn, wps,
                                                              _stream()))


# ================================================================================================ GRF and data path
@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("n0, n", [(64, 64), (256, 64)])
def test_grf_spectrum(n0, n, normalize, tag):
    import grf_ops as G
    from torch_cfd_amd.grf import GRF2d

    lib, B, real = _L(), 3, REAL[tag]
    torch.set_default_dtype(real)
    try:
        grf = GRF2d(n=n0, alpha=2.5, tau=7, device=_dev(), dtype=real, normalize=bool(normalize))
    finally:
        torch.set_default_dtype(torch.float32)
    noise = G.seeded_noise(11, B, n0, real).to(_dev())
    table = grf._device_table(n0, real, _dev())
    ref = torch.empty(B, n, n // 2 + 1, dtype=CPLX[tag], device=_dev())
    grf._spectrum(noise, n, ref)
    need = lib.tcfd_grf_spectrum_workspace_bytes(B, n, normalize)
    assert (need > 0) == bool(normalize)
    guard(f"tcfd_grf_spectrum normalize={normalize}", {"noise": noise, "table": table}, {"out": Out(CPLX[tag], (B, n, n // 2 + 1))},
          lambda P, ws, nb: lib.tcfd_grf_spectrum(P("noise"), P("table"), P("out"), B, n0, n, CODE[tag], normalize, ws, nb, _stream()),
          need, {"out": ref}, nullable_ws=True)      # normalize = 0: workspace = NULL and 0 bytes


DATA_DTYPES = [("f32", "f32"), ("f64", "f32"), ("f32", "f64")]


@pytest.mark.parametrize("src, dst", DATA_DTYPES, ids=[f"{a}-{b}" for a, b in DATA_DTYPES])
@pytest.mark.parametrize("n, out_steps, time_last", [(8, 5, 0), (12, 10, 1), (80, 5, 1), (80, 10, 0), (11, 5, 0), (11, 5, 1)])
def test_data_window(n, out_steps, time_last, src, dst):
    from torch_cfd_amd import datasets as D

    lib, rows, steps = _L(), 5, 3
    total = steps + out_steps + 4
    points = n * (n - 1) if n == 12 else n * n              # 12 x 11: a ragged 64-point tile; 11 x 11: an odd plane
    if n == 11:     # neither window is a whole number of 16-byte vectors, in either output type
        assert points % 2 == 1 and (points * steps) % 4 != 0 and (points * out_steps) % 4 != 0
    gen = torch.Generator().manual_seed(n)
    data = torch.randn(*((rows, points, total) if time_last else (rows, total, points)), generator=gen, dtype=REAL[src]).to(_dev())
    idx = torch.tensor([4, 0, 2, 2, 1], dtype=torch.int64)
    starts = torch.tensor([0, 4, 1, 3, 2], dtype=torch.int64)
    count = idx.numel()
    ref_in, ref_out = D._hip_window(data, torch.stack([idx, starts]).to(_dev()), steps, out_steps, bool(time_last), REAL[dst])
    ref_in, ref_out = ref_in.reshape(count, points, steps), ref_out.reshape(count, points, out_steps)
    call = lambda P, ws, nb: lib.tcfd_data_window(P("src"), P("a"), P("b"), P("idx"), P("starts"), count, rows, total, points, steps,
                                                  out_steps, time_last, CODE[src], CODE[dst], _stream())
    guard("tcfd_data_window", {"src": data, "idx": idx, "starts": starts},
          {"a": Out(REAL[dst], (count, points, steps)), "b": Out(REAL[dst], (count, points, out_steps))}, call, None,
          {"a": ref_in, "b": ref_out})
    # an entry outside the source "writes nothing for its sample": its slot keeps the poison, its neighbours are intact
    bad = idx.clone()
    bad[2] = rows
    skip = torch.zeros(count, dtype=torch.bool)
    skip[2] = True
    guard("tcfd_data_window with an out-of-range row", {"src": data, "idx": bad, "starts": starts},
          {"a": Out(REAL[dst], (count, points, steps), untouched=skip.to(_dev())),
           "b": Out(REAL[dst], (count, points, out_steps), untouched=skip.to(_dev()))}, call, None, {"a": ref_in, "b": ref_out})


@pytest.mark.parametrize("src, dst", DATA_DTYPES, ids=[f"{a}-{b}" for a, b in DATA_DTYPES])
@pytest.mark.parametrize("n, out_steps", [(8, 5), (12, 10), (80, 5), (9, 5), (11, 5)])
def test_data_fno3d_batch(n, out_steps, src, dst):
    from torch_cfd_amd import datasets as D

    lib, rows, steps = _L(), 4, 3
    if n % 2:       # an odd plane: no whole number of 16-byte vectors of either output type -- the scalar-store kernel and its tail
        assert (n * n * out_steps) % 4 != 0 and (n * n * out_steps) % 2 != 0
    gen = torch.Generator().manual_seed(n)
    field = torch.randn(rows, steps, n, n, generator=gen, dtype=REAL[src]).to(_dev())
    target = torch.randn(rows, n, n, out_steps, generator=gen, dtype=REAL[src]).to(_dev())
    idx = torch.tensor([3, 0, 2], dtype=torch.int64)
    count = idx.numel()
    grids = [torch.linspace(0, 1, k, dtype=REAL[dst]).to(_dev()) for k in (n, n, out_steps)]
    ref_in, ref_out = D._hip_fno3d_batch(field, target, idx.to(_dev()), grids, REAL[dst])
    ins = {"field": field, "target": target, "idx": idx, "gx": grids[0], "gy": grids[1], "gt": grids[2]}
    call = lambda P, ws, nb: lib.tcfd_data_fno3d_batch(P("field"), P("target"), P("idx"), P("gx"), P("gy"), P("gt"), P("inp"), P("out"),
                                                       count, rows, steps, n, out_steps, CODE[src], CODE[dst], _stream())
    shapes = ((count, 3 + steps, n, n, out_steps), (count, n, n, out_steps))
    guard("tcfd_data_fno3d_batch", ins, {"inp": Out(REAL[dst], shapes[0]), "out": Out(REAL[dst], shapes[1])}, call, None,
          {"inp": ref_in, "out": ref_out})
    bad = idx.clone()
    bad[1] = -1
    skip = torch.zeros(count, dtype=torch.bool)
    skip[1] = True
    guard("tcfd_data_fno3d_batch with an out-of-range row", {**ins, "idx": bad},
          {"inp": Out(REAL[dst], shapes[0], untouched=skip.to(_dev())), "out": Out(REAL[dst], shapes[1], untouched=skip.to(_dev()))},
          call, None, {"inp": ref_in, "out": ref_out})


@pytest.mark.parametrize("mode", [0, 1])
def test_data_affine(mode):
    from torch_cfd_amd import datasets as D

    lib, eps = _L(), 1e-5
    gen = torch.Generator().manual_seed(2)
    rows, stat_count, inner = 3, 7, 11                        # total = 231: no multiple of any vector width
    for xt, st, ot in (("f32", "f32", "f32"), ("f64", "f32", "f64"), ("f32", "f64", "f32"), ("f32", "f32", "f64")):
        x = torch.randn(rows, stat_count, inner, generator=gen, dtype=REAL[xt]).to(_dev())
        mean = torch.randn(stat_count, generator=gen, dtype=REAL[st]).to(_dev())
        std = (torch.rand(stat_count, generator=gen, dtype=REAL[st]) + 0.5).to(_dev())
        total = x.numel()
        for mean_t in (mean, None):
            ref = D._hip_affine(x, mean_t, std, eps, mode, inner, REAL[ot])
            ins = {"x": x, "std": std, **({"mean": mean} if mean_t is not None else {})}
            call = lambda P, ws, nb, o: lib.tcfd_data_affine(P("x"), P("mean") if mean_t is not None else None, P("std"), P(o), total,
                                                             stat_count, inner, eps, mode, CODE[xt], CODE[st], CODE[ot], _stream())
            guard(f"tcfd_data_affine {xt}/{st}->{ot}", ins, {"out": Out(REAL[ot], tuple(x.shape))},
                  lambda P, ws, nb: call(P, ws, nb, "out"), None, {"out": ref})
            if xt == ot:
                guard(f"tcfd_data_affine {xt}/{st} in place", ins, {"x": Out(REAL[ot], tuple(x.shape))},
                      lambda P, ws, nb: call(P, ws, nb, "x"), None, {"x": ref})


@pytest.mark.parametrize("xt, st", DATA_DTYPES, ids=[f"{a}-{b}" for a, b in DATA_DTYPES])
@pytest.mark.parametrize("spatial, shape", [(False, (9, 5, 7)), (True, (6, 3, 5, 77)), (True, (4, 130, 100))])
def test_data_moments(spatial, shape, xt, st):
    from torch_cfd_amd import datasets as D

    lib = _L()
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(len(shape)), dtype=REAL[xt]).to(_dev())
    mean, std = D._hip_moments(x, spatial, REAL[st])
    rows, inner = shape[0], (shape[-1] if spatial else 1)
    count = x.numel() // (rows * inner)
    assert inner == 1 or inner % 64 != 0
    o = Out(REAL[st], tuple(mean.shape))
    guard(f"tcfd_data_moments inner={inner}", {"x": x}, {"mean": o, "std": o},
          lambda P, ws, nb: lib.tcfd_data_moments(P("x"), P("mean"), P("std"), rows, count, inner, CODE[xt], CODE[st], _stream()),
          None, {"mean": mean, "std": std})


# ================================================================================================ FNO transforms and contraction
FNO_PLANS = [(16, 16, 10, (4, 4, 3), "f32", True), (32, 64, 7, (8, 8, 4), "f32", True), (96, 96, 6, (8, 8, 3), "f32", True),
             (20, 28, 6, (4, 4, 3), "f32", False), (16, 16, 10, (4, 4, 3), "f64", True)]


def _crandn(gen, tag, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=gen, dtype=CPLX[tag])).to(_dev())


def _ptr4(P, prefix):
    return (ctypes.c_void_p * 4)(*[P(f"{prefix}{k}") for k in range(4)])


@pytest.mark.parametrize("X, Y, T, modes, tag, fft", FNO_PLANS, ids=[f"{p[0]}x{p[1]}x{p[2]}-{p[4]}-{'fft' if p[5] else 'dft'}" for p in FNO_PLANS])
def test_fno_transforms(X, Y, T, modes, tag, fft):
    from torch_cfd_amd import fno

    lib, real = _L(), REAL[tag]
    b, ci, co, t_pad, delta = 2, 3, 5, 2, 0.05
    t_out = T + t_pad
    t_keep = T - 1 if T % 2 == 0 else T - 2
    assert t_keep % 2 == 1
    assert (fno._fft_len(X) and fno._fft_len(Y)) == fft            # FFT kernels, or the pruned direct DFTs
    mx, my, mt = modes
    plan = fno._plan((X, Y, T, t_pad, t_out) + modes, _dev(), real)
    h = plan.handle
    assert lib.tcfd_fno_plan_supports(h, t_keep) == 1
    assert lib.tcfd_fno_workspace_bytes(h, 0, ci, co) == 0
    fs, is_ = fno._norm_scales("backward", X * Y * (T + t_pad), X * Y * t_out)
    gen = torch.Generator().manual_seed(X + T)
    v = torch.randn(b, ci, X, Y, T, generator=gen, dtype=real).to(_dev())
    W = [_crandn(gen, tag, ci, co, mx, my, mt, scale=0.1) for _ in range(4)]
    Bz = [_crandn(gen, tag, mx, my, mt) for _ in range(4)]
    params = {**{f"w{k}": W[k] for k in range(4)}, **{f"b{k}": Bz[k] for k in range(4)}}
    out5 = Out(real, (b, co, X, Y, t_keep))
    need = lib.tcfd_fno_workspace_bytes(h, b, ci, co)
    for mfma in (0, 1):
        ref = fno.hip_spectral_conv(v, W, Bz, delta, modes, t_pad=t_pad, t_out=t_out, t_keep=t_keep, use_mfma=bool(mfma))
        guard(f"tcfd_fno_spectral_conv use_mfma={mfma}", {"v": v, **params}, {"out": out5},
              lambda P, ws, nb: lib.tcfd_fno_spectral_conv(h, P("v"), _ptr4(P, "w"), _ptr4(P, "b"), delta, P("out"), b, ci, co, t_keep,
                                                           fs, is_, mfma, ws, nb, _stream()),
              need, {"out": ref})
    # the two halves: forward with c = cin, inverse with c = cout
    kts = fno._c2r_weights(mt, t_out, _dev(), real)
    need_i = lib.tcfd_fno_workspace_bytes(h, b, ci, ci)
    vh_o = Out(CPLX[tag], (b, ci, 2 * mx, 2 * my, mt))
    ref_vh = fno.hip_truncated_rfftn(v, modes, t_pad=t_pad, t_out=t_out)[0]
    guard("tcfd_fno_forward_trunc", {"v": v}, {"vh": vh_o},
          lambda P, ws, nb: lib.tcfd_fno_forward_trunc(h, P("v"), P("vh"), b, ci, fs, ws, nb, _stream()), need_i, {"vh": ref_vh})
    guard("tcfd_fno_forward_trunc_kt", {"v": v, "kt": kts}, {"vh": vh_o},
          lambda P, ws, nb: lib.tcfd_fno_forward_trunc_kt(h, P("v"), P("vh"), b, ci, fs, P("kt"), ws, nb, _stream()),
          need_i, {"vh": fno.hip_truncated_rfftn(v, modes, t_pad=t_pad, t_out=t_out, kt_scale=kts)[0]})
    vh = _crandn(gen, tag, b, co, 2 * mx, 2 * my, mt)
    acc = torch.randn(b, co, X, Y, t_keep, generator=gen, dtype=real).to(_dev())
    last = torch.randn(b, co, X, Y, generator=gen, dtype=real).to(_dev())
    res = torch.randn(b * co, X, Y, T, generator=gen, dtype=real).to(_dev())
    need_o = lib.tcfd_fno_workspace_bytes(h, b, co, co)
    irf = lambda **kw: fno.hip_truncated_irfftn(vh, plan, t_keep, **kw)
    guard("tcfd_fno_inverse_trunc", {"vh": vh}, {"out": out5},
          lambda P, ws, nb: lib.tcfd_fno_inverse_trunc(h, P("vh"), P("out"), b, co, t_keep, is_, ws, nb, _stream()),
          need_o, {"out": irf()})
    guard("tcfd_fno_inverse_trunc_acc acc == out", {"vh": vh, "out": acc}, {"out": out5},
          lambda P, ws, nb: lib.tcfd_fno_inverse_trunc_acc(h, P("vh"), P("out"), P("out"), b, co, t_keep, is_, ws, nb, _stream()),
          need_o, {"out": irf(accumulate=acc.clone())})
    guard("tcfd_fno_inverse_trunc_last", {"vh": vh, "last": last}, {"out": out5},
          lambda P, ws, nb: lib.tcfd_fno_inverse_trunc_last(h, P("vh"), P("out"), P("last"), b, co, t_keep, is_, ws, nb, _stream()),
          need_o, {"out": irf(add_last=last)})
    call = lambda P, ws, nb: lib.tcfd_fno_inverse_trunc_residual(h, P("vh"), P("out"), P("res"), T, b, co, t_keep, is_, ws, nb, _stream())
    guard("tcfd_fno_inverse_trunc_residual", {"vh": vh, "res": res}, {"out": out5}, call, need_o,
          roomy({"vh": vh, "res": res}, {"out": out5}, call, need_o))      # (its wrapper is inline in OutConv.forward, c = 1)
    guard("tcfd_fno_inverse_trunc_kt", {"vh": vh, "kt": kts}, {"out": out5},
          lambda P, ws, nb: lib.tcfd_fno_inverse_trunc_kt(h, P("vh"), P("out"), None, None, b, co, t_keep, is_, P("kt"), ws, nb, _stream()),
          need_o, {"out": irf(kt_scale=kts)})
    guard("tcfd_fno_inverse_trunc_kt acc == out", {"vh": vh, "kt": kts, "out": acc}, {"out": out5},
          lambda P, ws, nb: lib.tcfd_fno_inverse_trunc_kt(h, P("vh"), P("out"), P("out"), None, b, co, t_keep, is_, P("kt"), ws, nb,
                                                          _stream()),
          need_o, {"out": irf(kt_scale=kts, accumulate=acc.clone())})


def test_fno_resample():
    """An inverse plan onto a 32 x 32 grid of a spectrum taken on 16 x 16: only tcfd_fno_inverse_trunc may be called with it."""
    from torch_cfd_amd import fno

    lib, tag, b, c = _L(), "f32", 2, 5
    X, Y, T, modes, t_keep = 32, 32, 10, (4, 4, 3), 7
    plan = fno._plan((X, Y, T, 0, T) + modes + (16, 16), _dev(), REAL[tag])
    _, is_ = fno._norm_scales("backward", X * Y * T, X * Y * T)
    vh = _crandn(torch.Generator().manual_seed(8), tag, b, c, 2 * modes[0], 2 * modes[1], modes[2])
    need = lib.tcfd_fno_workspace_bytes(plan.handle, b, c, c)
    guard("tcfd_fno_inverse_trunc (resample plan)", {"vh": vh}, {"out": Out(REAL[tag], (b, c, X, Y, t_keep))},
          lambda P, ws, nb: lib.tcfd_fno_inverse_trunc(plan.handle, P("vh"), P("out"), b, c, t_keep, is_, ws, nb, _stream()),
          need, {"out": fno.hip_truncated_irfftn(vh, plan, t_keep)})


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("b, ci, co, modes", [(3, 1, 1, (2, 2, 4)), (17, 33, 20, (4, 2, 2))])
def test_fno_contract(b, ci, co, modes, tag):
    from torch_cfd_amd import fno

    lib, delta = _L(), 0.05
    mx, my, mt = modes
    gen = torch.Generator().manual_seed(b)
    vh = _crandn(gen, tag, b, ci, 2 * mx, 2 * my, mt)
    gh = _crandn(gen, tag, b, co, 2 * mx, 2 * my, mt)
    W = [_crandn(gen, tag, ci, co, mx, my, mt, scale=0.1) for _ in range(4)]
    Bz = [_crandn(gen, tag, mx, my, mt) for _ in range(4)]
    wins = {f"w{k}": W[k] for k in range(4)}
    bins = {f"b{k}": Bz[k] for k in range(4)}
    spec = lambda c: Out(CPLX[tag], (b, c, 2 * mx, 2 * my, mt))
    for mfma in (0, 1):
        guard(f"tcfd_fno_contract use_mfma={mfma}", {"vh": vh, **wins, **bins}, {"out": spec(co)},
              lambda P, ws, nb: lib.tcfd_fno_contract(P("vh"), _ptr4(P, "w"), _ptr4(P, "b"), delta, P("out"), b, ci, co, mx, my, mt,
                                                      mfma, CODE[tag], _stream()),
              None, {"out": fno.hip_contract(vh, W, Bz, delta, modes, use_mfma=bool(mfma))})
        gv, _ = fno._contract_vjp(gh, vh, W + Bz, (delta, modes, bool(mfma), True), True, [False] * 8)
        guard(f"tcfd_fno_contract_adjoint use_mfma={mfma}", {"gh": gh, **wins}, {"gv": spec(ci)},
              lambda P, ws, nb: lib.tcfd_fno_contract_adjoint(P("gh"), _ptr4(P, "w"), P("gv"), b, co, ci, mx, my, mt, mfma, CODE[tag],
                                                              _stream()),
              None, {"gv": gv})
    _, grads = fno._contract_vjp(gh, vh, W + Bz, (delta, modes, True, True), False, [True] * 8)
    gw_o = {f"gw{k}": Out(CPLX[tag], (ci, co, mx, my, mt)) for k in range(4)}
    gb_o = {f"gb{k}": Out(CPLX[tag], (mx, my, mt)) for k in range(4)}
    ref = {**{f"gw{k}": grads[k] for k in range(4)}, **{f"gb{k}": grads[4 + k] for k in range(4)}}
    guard("tcfd_fno_contract_wgrad", {"vh": vh, "gh": gh}, {**gw_o, **gb_o},
          lambda P, ws, nb: lib.tcfd_fno_contract_wgrad(P("vh"), P("gh"), _ptr4(P, "gw"), _ptr4(P, "gb"), delta, b, ci, co, mx, my, mt,
                                                        CODE[tag], _stream()),
          None, ref)
    guard("tcfd_fno_contract_wgrad gb=NULL", {"vh": vh, "gh": gh}, gw_o,
          lambda P, ws, nb: lib.tcfd_fno_contract_wgrad(P("vh"), P("gh"), _ptr4(P, "gw"), None, delta, b, ci, co, mx, my, mt, CODE[tag],
                                                        _stream()),
          None, {k: ref[k] for k in gw_o})


# ================================================================================================ pointwise blocks
PW_SHAPES = {540: (6, 9, 10), 630: (7, 9, 10)}       # P = X * Y * T: P % 16 = 12 (ragged MFMA tile), P % 4 = 2 (vector kernel)


def _pw_block(width, P, act, mode, tag):
    """One block ci -> 4 ci -> ci as the layers build it (1x1x1 convolutions), its inputs, and the kernel's operands through
    the package's own marshalling (fno._pointwise_operands)."""
    import torch.nn as nn
    from torch_cfd_amd import fno

    real = REAL[tag]
    ci = co = width
    cm = 4 * ci
    mk = lambda i, o: nn.Conv3d(i, o, 1).to(device=_dev(), dtype=real)
    with torch.random.fork_rng(devices=[]):      # the modules draw their weights from the global generator: leave it as it was
        torch.manual_seed(width + P)
        lin1, lin2 = mk(ci, cm), mk(cm, co)
        skip_conv = mk(ci, co) if mode == 1 else None
    b, (X, Y, T), sT = 2, PW_SHAPES[P], 3
    gen = torch.Generator().manual_seed(P + mode)
    x = torch.randn(b, ci, X, Y, T, generator=gen, dtype=real).to(_dev())
    skip = torch.randn(*((b, ci, X, Y, T) if mode == 1 else (b, co, X, Y, sT)), generator=gen, dtype=real).to(_dev())
    actm = {"gelu": nn.GELU, "relu": nn.ReLU}[act]()
    names = ("w1", "b1", "w2t", "b2", "wst", "bs")
    ops = {k: t for k, t in zip(names, fno._pointwise_operands(lin1, lin2, skip_conv)) if t is not None}
    dims = dict(b=b, ci=ci, cm=cm, co=co, P=P, T=T, sT=sT if mode == 2 else 0, c=fno._act_code(actm), mode=mode)
    return lin1, lin2, skip_conv, actm, x, skip, ops, dims


PW_CASES = [(w, P, act, mode) for w in (10, 16) for P in (540, 630) for act in ("gelu", "relu") for mode in (1, 2)]


@pytest.mark.parametrize("width, P, act, mode", PW_CASES)
def test_fno_pointwise(width, P, act, mode):
    from torch_cfd_amd import fno

    assert 540 % 16 == 12 and 630 % 4 == 2 and P in PW_SHAPES
    lib = _L()
    lin1, lin2, skip_conv, actm, x, skip, ops, d = _pw_block(width, P, act, mode, "f32")
    b, ci, cm, co, T, sT, c = d["b"], d["ci"], d["cm"], d["co"], d["T"], d["sT"], d["c"]
    z2 = torch.empty(b, co, *x.shape[2:], dtype=torch.float32, device=_dev())
    with torch.no_grad():
        ref = fno.hip_pointwise(x, lin1, actm, lin2, skip=skip, skip_conv=skip_conv, act2=actm, skip_last_slice=(mode == 2), pre=z2)
    assert ref is not None, "the block is not instantiated"
    o = Out(torch.float32, tuple(ref.shape))
    ins = {"x": x, "skip": skip, **ops}
    opt = lambda P_, k: P_(k) if k in ops else None
    tail = (b, ci, cm, co, P, T, sT, c, c, mode, 0, 0, None)
    guard("tcfd_fno_pointwise", ins, {"out": o},
          lambda P_, ws, nb: lib.tcfd_fno_pointwise(P_("x"), P_("skip"), P_("out"), P_("w1"), P_("b1"), P_("w2t"), P_("b2"),
                                                    opt(P_, "wst"), opt(P_, "bs"), *tail, _stream()),
          None, {"out": ref})
    guard("tcfd_fno_pointwise_pre", ins, {"out": o, "pre": o},
          lambda P_, ws, nb: lib.tcfd_fno_pointwise_pre(P_("x"), P_("skip"), P_("out"), P_("pre"), P_("w1"), P_("b1"), P_("w2t"), P_("b2"),
                                                        opt(P_, "wst"), opt(P_, "bs"), *tail, _stream()),
          None, {"out": ref, "pre": z2})
    # backward with what the forward kept
    spec = (True, actm, actm, mode, None)
    kind = fno._saved_kind(spec, ci, cm, co, P)
    kept = {0: None, 1: ref, 2: z2}[kind]
    layout = fno._pointwise_bwd_layout(True, b, ci, cm, co, P, T, sT, c, c, mode)
    if layout is None:
        # The backward kernels cover width 16 only on the tiled kernel, which needs P % 4 == 0 (the layers then differentiate the
        # block with torch operations): the vector-ragged P reaches tcfd_fno_pointwise_bwd_out at width 10 alone.  Nothing else
        # may be missing.
        assert (width, P) == (16, 630), "the pointwise backward is not instantiated for a shape the layers use"
        return
    per_row = layout[4]
    dout = torch.randn(*ref.shape, generator=torch.Generator().manual_seed(3)).to(_dev())
    hip = fno._hip_pointwise_backward(spec, dout, x, skip, lin1.weight, lin1.bias, lin2.weight, lin2.bias,
                                      skip_conv.weight if mode == 1 else None, skip_conv.bias if mode == 1 else None, None, None,
                                      need_dx=True, out=kept)
    assert hip is not None
    max_waves = max(2048, int(layout[5]))
    ds_shape = tuple(skip.shape) if mode == 1 else tuple(ref.shape)
    bins = {**ins, "dout": dout, **({"kept": kept} if kept is not None else {})}
    written = []

    def bwd(P_, ws, nb):
        dims = (ctypes.c_int * 6)(*layout)
        rc = lib.tcfd_fno_pointwise_bwd_out(P_("x"), P_("skip"), P_("dout"), P_("kept") if kept is not None else None, P_("dx"), P_("ds"),
                                            P_("w1"), P_("b1"), P_("w2t"), P_("b2"), opt(P_, "wst"), opt(P_, "bs"), P_("partials"),
                                            max_waves, dims, b, ci, cm, co, P, T, sT, c, c, mode, 0, _stream())
        assert rc != 0 or tuple(dims)[:5] == tuple(layout)[:5]
        written.append(int(dims[5]))
        return rc

    # `partials` is POISONED, not zeroed as the wrapper does: what a launch stores is part of the contract (include/tcfd.h).  Rows
    # behind dims[5] are never written.  In the rows of its waves the LDS-staged kernel (P % 4 != 0) stores everything, padding as
    # zeros; the tiled all-MFMA kernel (P % 4 == 0) stores exactly the entries that mean something -- A[o < co][dW2 | db2 | dWs with a
    # skip convolution], B[m < cm][dW1 | db1] -- and leaves the padding to the caller, who zero-fills the buffer first.
    COP, CB, CM1, CIP = (int(v) for v in layout[:4])
    assert per_row == COP * CB + CM1 * CIP
    means = torch.zeros(per_row, dtype=torch.bool)
    means[:COP * CB].view(COP, CB)[:co, :cm + 1 + (ci if mode == 1 else 0)] = True
    means[COP * CB:].view(CM1, CIP)[:cm, :ci + 1] = True
    bouts = {"dx": Out(torch.float32, tuple(x.shape)), "ds": Out(torch.float32, ds_shape),
             "partials": Out(torch.float32, (max_waves, per_row))}
    ref_b = roomy(bins, bouts, bwd)
    rows = written[0]
    assert 0 < rows <= max_waves
    idle = torch.zeros(max_waves, per_row, dtype=torch.bool)
    idle[rows:] = True
    if P % 4 == 0:
        idle[:, ~means] = True
    bouts["partials"] = Out(torch.float32, (max_waves, per_row), untouched=idle.to(_dev()))
    assert torch.equal(ref_b["dx"], hip[0])                 # ... and the wrapper hands that dx on (and ds, where it is the skip gradient)
    if mode == 1:
        assert torch.equal(ref_b["ds"], hip[1])
    got = guard("tcfd_fno_pointwise_bwd_out", bins, bouts, bwd, None, ref_b)
    assert set(written) == {rows}
    if P % 4 != 0:          # whole rows: the padding is exact zeros
        assert not bool(got["partials"][:rows][:, ~means.to(_dev())].any())


@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("width, P", [(10, 540), (10, 630), (16, 540), (16, 630)])
def test_fno_pointwise_f64(width, P, mode, act):
    from torch_cfd_amd import fno

    lib = _L()
    lin1, lin2, skip_conv, actm, x, skip, ops, d = _pw_block(width, P, act, mode, "f64")
    with torch.no_grad():
        ref = fno.hip_pointwise(x, lin1, actm, lin2, skip=skip, skip_conv=skip_conv, act2=actm, skip_last_slice=(mode == 2))
    assert ref is not None and ref.dtype == torch.float64
    opt = lambda P_, k: P_(k) if k in ops else None
    guard("tcfd_fno_pointwise_f64", {"x": x, "skip": skip, **ops}, {"out": Out(torch.float64, tuple(ref.shape))},
          lambda P_, ws, nb: lib.tcfd_fno_pointwise_f64(P_("x"), P_("skip"), P_("out"), P_("w1"), P_("b1"), P_("w2t"), P_("b2"),
                                                        opt(P_, "wst"), opt(P_, "bs"), d["b"], d["ci"], d["cm"], d["co"], P, d["T"],
                                                        d["sT"], d["c"], d["c"], mode, 0, 0, _stream()),
          None, {"out": ref})


@pytest.mark.parametrize("C, co, P", [(10, 10, 540), (10, 10, 630), (16, 16, 540), (16, 16, 630)])
def test_fno_pointwise_bwd_pe(C, co, P):
    """The per-sample weight-gradient sums of the lifting projection (x1 + pe), as fno._hip_norm_proj_backward calls it: no dx,
    max_waves = 2048 + b rows of which the launch reports how many it wrote -- the others must stay untouched."""
    lib, b = _L(), 3
    gen = torch.Generator().manual_seed(C + P)
    x1, pe, dout = torch.randn(b, P, generator=gen), torch.randn(C, P, generator=gen), torch.randn(b, co, P, generator=gen)
    w2t = torch.randn(C, co, generator=gen)
    query = (ctypes.c_int * 6)()
    assert lib.tcfd_fno_pointwise_bwd(None, None, None, None, None, None, None, None, None, None, None, None, 0, query, b, C, C, co, P, 0,
                                      0, 0, 0, 0, 1, None) == 0
    per_row, max_waves = query[4], 2048 + b
    written = []

    def call(P_, ws, nb):
        dims = (ctypes.c_int * 6)(*query)
        rc = lib.tcfd_fno_pointwise_bwd_pe(P_("x1"), P_("pe"), P_("dout"), None, P_("w2t"), None, P_("partials"), max_waves, dims, b, C,
                                           co, P, 1, _stream())
        written.append(int(dims[5]))
        return rc

    ins = {"x1": x1, "pe": pe, "dout": dout, "w2t": w2t}
    ref = roomy(ins, {"partials": Out(torch.float32, (max_waves, per_row))}, call)
    rows = written[0]
    assert 0 < rows <= max_waves and rows % b == 0
    idle = torch.arange(max_waves, device=_dev()) >= rows
    guard("tcfd_fno_pointwise_bwd_pe", ins, {"partials": Out(torch.float32, (max_waves, per_row), untouched=idle)}, call, None, ref)
    assert set(written) == {rows}
