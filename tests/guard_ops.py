"""Guard harness for the raw-pointer C ABI (test-only, plain torch on whatever device it is given; no kernels of its own).

One ordinary allocation -- the arena -- holds every buffer of a call at a 256-byte-aligned offset, with moats of a known byte
value between and around them.  A call that writes outside what it was given damages a moat; a call that forgets to store an
output element leaves the poison there; a call whose result depends on scratch it never wrote gives different bits when the
poison changes.  ``run_guarded`` is the one protocol every case goes through (tests/test_memory_contract_gpu.py); the planted
defects of tests/test_guard_host.py show that it sees what it claims to see.

What it cannot see: a load past the end of an input whose value is masked out before it reaches a result (the arena is one
allocation, so such a load does not fault either), and a stray write that happens to store the poison value.  Two poison values
(0xFF, then 0x00) cover the second for every byte that is not written as both; a third run leaves the workspace as the call
before dirtied it, for a kernel that would lean on its own leftovers.
"""
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

ALIGN = 256                 # what hipMalloc promises and align256 in the library assumes
EDGE = 16 << 20             # head and tail moat: at least this, and at least the largest region
TCFD_EWORKSPACE = -4
POISONS = (0xFF, 0x00)      # every float32 / float64 made of 0xFF bytes is a NaN


def _up(x: int, a: int = ALIGN) -> int:
    return (x + a - 1) // a * a


def nbytes(dtype: torch.dtype, shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n * torch.empty((), dtype=dtype).element_size()


class Arena:
    """``regions``: ordered (name, nbytes).  Usable length of a region is exactly nbytes: the slack up to the next 256-byte
    boundary belongs to the moat behind it."""

    def __init__(self, device, regions: Sequence[Tuple[str, int]], moat: int = 1 << 20):
        self.device = torch.device(device)
        self.names = [r[0] for r in regions]
        assert len(set(self.names)) == len(self.names), "region names must be unique"
        self.size: Dict[str, int] = {name: int(nb) for name, nb in regions}
        assert all(v >= 0 for v in self.size.values())
        edge = _up(max([EDGE] + list(self.size.values())))
        moat = _up(max(int(moat), ALIGN))
        self.offset: Dict[str, int] = {}
        pos = edge
        for i, name in enumerate(self.names):
            if i:
                pos += moat
            self.offset[name] = pos
            pos = _up(pos + self.size[name])
        self.total = pos + edge
        # over-allocate by one alignment unit so that the base of the arena itself sits on a 256-byte boundary
        self._raw = torch.empty(self.total + ALIGN, dtype=torch.uint8, device=self.device)
        shift = (-self._raw.data_ptr()) % ALIGN
        self.buf = self._raw[shift:shift + self.total]
        assert self.buf.data_ptr() % ALIGN == 0
        self.is_moat = torch.ones(self.total, dtype=torch.bool, device=self.device)
        for name in self.names:
            self.is_moat[self.offset[name]:self.offset[name] + self.size[name]] = False

    # -- addressing
    def ptr(self, name: str) -> int:
        return self.buf.data_ptr() + self.offset[name]

    def raw(self, name: str) -> torch.Tensor:
        return self.buf[self.offset[name]:self.offset[name] + self.size[name]]

    def view(self, name: str, dtype: torch.dtype, shape) -> torch.Tensor:
        nb = nbytes(dtype, shape)
        assert nb <= self.size[name], f"region {name}: view of {nb} bytes in {self.size[name]}"
        return self.raw(name)[:nb].view(dtype).view(*shape)

    # -- poison and checks
    def poison(self, byte: int, keep: Sequence[str] = ()) -> None:
        """Fill the moats and every region not named in ``keep`` (the inputs) with ``byte``."""
        saved = {k: self.raw(k).clone() for k in keep}
        self.buf.fill_(byte)
        for k, v in saved.items():
            self.raw(k).copy_(v)

    def adjoining(self, off: int) -> str:
        """Which region a moat offset adjoins, and on which side."""
        best, text = None, "nothing"
        for name in self.names:
            lo, hi = self.offset[name], self.offset[name] + self.size[name]
            for dist, side in ((lo - off, "before"), (off - hi + 1, "past the end of")):
                if dist > 0 and (best is None or dist < best):
                    best, text = dist, f"{dist} byte(s) {side} region '{name}'"
        return text

    def moats_intact(self, byte: int) -> Tuple[bool, str]:
        """One device-side comparison over all moat bytes; on failure the first and last damaged offset."""
        bad = (self.buf != byte) & self.is_moat
        if not bool(bad.any()):
            return True, ""
        idx = bad.nonzero().flatten()
        first, last = int(idx[0]), int(idx[-1])
        return False, (f"{idx.numel()} moat byte(s) changed from 0x{byte:02X}: first at arena offset {first} ({self.adjoining(first)}), "
                       f"last at {last} ({self.adjoining(last)})")


@dataclass
class Out:
    """An output region: its element type and shape, and optionally ``untouched`` -- a bool mask (or an index expression) of
    the elements the contract says the call must NOT write (they keep the poison)."""
    dtype: torch.dtype
    shape: tuple
    untouched: Optional[object] = None


def _real(t: torch.Tensor) -> torch.Tensor:
    return torch.view_as_real(t) if t.is_complex() else t


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(-1).view(torch.uint8)


def _written_mask(o: Out, device) -> Optional[torch.Tensor]:
    if o.untouched is None:
        return None
    m = torch.ones(o.shape, dtype=torch.bool, device=device)
    m[o.untouched] = False
    return m


class GuardError(AssertionError):
    pass


def run_guarded(call: Callable[[int], int], arena: Arena, inputs: Dict[str, torch.Tensor], outputs: Dict[str, Out],
                workspace: Optional[str] = None, *, need: Optional[int] = None, baseline: Optional[Dict[str, torch.Tensor]] = None,
                last_error: Optional[Callable[[], bytes]] = None, sync: Optional[Callable[[], None]] = None,
                what: str = "call") -> Dict[str, torch.Tensor]:
    """``call(ws_bytes)`` makes the call under test on the arena's pointers, passing ``ws_bytes`` as the workspace size, and
    returns its status.  ``inputs``: region -> tensor copied in before each run.  ``outputs``: region -> Out.  A region named in
    both is an allowed alias (in-place call): it is loaded like an input and checked like an output.  ``workspace``: the scratch
    region (``need`` bytes are passed; default its whole length) or None.  ``baseline``: region -> the same result by the roomy
    wrapper path.  Three runs (0xFF poison, 0x00 poison, 0x00 poison around a workspace still dirty from the run before) must
    give the same bits; a last call with ``need - 1`` bytes must refuse and touch nothing.  Returns the outputs of the first run."""
    dev = arena.device
    sync = sync or (torch.cuda.synchronize if dev.type == "cuda" else (lambda: None))
    need = (arena.size[workspace] if workspace else 0) if need is None else need
    pure_inputs = [k for k in inputs if k not in outputs]

    def fail(msg):
        raise GuardError(f"{what}: {msg}")

    def load(byte, keep=()):
        arena.poison(byte, keep=keep)
        for k, t in inputs.items():
            src = _bits(t.to(dev))
            if src.numel() != arena.size[k]:
                fail(f"input region '{k}' is {arena.size[k]} bytes, its data {src.numel()}")
            arena.raw(k).copy_(src)

    def check_bystanders(byte):
        ok, msg = arena.moats_intact(byte)
        if not ok:
            fail(msg)
        for k in pure_inputs:
            if not torch.equal(arena.raw(k), _bits(inputs[k].to(dev))):
                d = (arena.raw(k) != _bits(inputs[k].to(dev))).nonzero().flatten()
                fail(f"read-only input region '{k}' was modified ({d.numel()} bytes, first at +{int(d[0])})")

    # 0xFF everywhere; 0x00 everywhere; 0x00 in moats and outputs with the workspace left as the previous call dirtied it
    states = [(b, False) for b in POISONS] + ([(0x00, True)] if workspace is not None and need > 0 else [])
    results = []
    for byte, dirty in states:
        load(byte, keep=[workspace] if dirty else ())
        rc = call(need)
        sync()
        if rc != 0:
            fail(f"returned {rc} with exactly the workspace it asked for ({need} bytes)"
                 + (f": {last_error()!r}" if last_error else ""))
        check_bystanders(byte)
        got = {}
        for k, o in outputs.items():
            v = arena.view(k, o.dtype, o.shape)
            mask = _written_mask(o, dev)
            if mask is not None:
                kept = _bits(v[~mask])
                if not bool((kept == byte).all()):
                    fail(f"output region '{k}': elements the contract leaves alone were written")
            if v.is_floating_point() or v.is_complex():
                r = _real(v)
                nf = ~torch.isfinite(r)
                if mask is not None:
                    nf = nf & (mask.unsqueeze(-1) if v.is_complex() else mask)
                if bool(nf.any()):
                    idx = nf.nonzero()
                    fail(f"output region '{k}': {idx.shape[0]} element(s) not finite after the run on 0x{byte:02X} poison (unwritten, or "
                         f"computed from poisoned scratch); first at index {tuple(int(i) for i in idx[0])}")
            got[k] = v.clone()
        results.append(got)

    for k, o in outputs.items():
        mask = _written_mask(o, dev)
        a = results[0][k] if mask is None else results[0][k][mask]
        for other, label in zip(results[1:], ("the 0x00 run", "the run on a dirty workspace")):
            b = other[k] if mask is None else other[k][mask]
            if not torch.equal(_bits(a), _bits(b)):
                n = int((_real(a) != _real(b)).sum()) if a.numel() else 0
                fail(f"output region '{k}' differs between the 0xFF run and {label} ({n} element parts): the result depends on "
                     "memory the call never wrote")
        if baseline is not None and k in baseline:
            ref = baseline[k].to(dev)
            if tuple(ref.shape) != tuple(o.shape) or ref.dtype != o.dtype:
                fail(f"baseline of '{k}' is {tuple(ref.shape)} {ref.dtype}, the guarded output {tuple(o.shape)} {o.dtype}")
            if mask is not None:
                ref = ref[mask]
            if not torch.equal(_bits(a), _bits(ref)):
                d = _real(a).double() - _real(ref).double()
                fail(f"output region '{k}' is not bit-equal to the wrapper path: {int((d != 0).sum())} element parts differ, "
                     f"max |diff| {float(d.abs().max()):.3e}")

    if workspace is not None and need > 0:
        byte = 0xFF
        load(byte)
        rc = call(need - 1)
        sync()
        if rc != TCFD_EWORKSPACE:
            fail(f"returned {rc}, not TCFD_EWORKSPACE, with {need - 1} of {need} workspace bytes")
        if last_error is not None and not last_error():
            fail("TCFD_EWORKSPACE without a message in tcfd_last_error()")
        check_bystanders(byte)
        for k, o in outputs.items():
            want = _bits(inputs[k].to(dev)) if k in inputs else None
            raw = arena.raw(k)
            if not (torch.equal(raw, want) if want is not None else bool((raw == byte).all())):
                fail(f"output region '{k}' was touched by a call that returned TCFD_EWORKSPACE")
        if not bool((arena.raw(workspace) == byte).all()):
            fail(f"workspace region '{workspace}' was touched by a call that returned TCFD_EWORKSPACE")
    return results[0]
