"""Does any result depend on what an uninitialised buffer held?  (A plain helper module, not a conftest.)

alloc_fill(byte)            context manager: while it is active torch.empty, torch.empty_like, torch.empty_strided and
                            Tensor.new_empty return their normal tensor with EVERY byte of its storage set to `byte` -- on any
                            device, pinned host memory included, non-contiguous results through their storage.  The package calls
                            these through the torch module attribute at call time, so the patch reaches every allocation site
                            without touching product code.  The originals come back on exit, also when the body raises.
run_under_fills(fn)         fn() under 0x00 twice (the control: what a fresh process usually sees), then under 0xFF (NaN in f32,
                            f64, bf16 and f16, -1 in the integer types; also the library's own hand-off poison) and under 0x47
                            (finite and large: 51015.28 in f32, 50944 in bf16, 7.28 in f16, 1195853639 in int32 -- for the places
                            where a NaN is swallowed: fmaxf, ReLU, a compare, a clamp).  fn builds its model or object afresh on
                            every call and returns {name: tensor}; the four results come back as dicts of CPU tensors.
assert_fill_independent     the comparison rule: every named output of the 0xFF and of the 0x47 run equals the control
                              * BITWISE (torch.equal on the raw bits) wherever the two control runs are bitwise equal to each other;
                              * where the two control runs differ (float atomics): within twice the spread measured between them,
                                capped at 1e-3 of the tensor's largest absolute entry, and no NaN or Inf where the control has none.
                            masks: {name: bool tensor, True = compared} for regions the CONTRACT leaves unspecified; the masked
                            share of an output must stay below one half.  Returns {name: control-to-control spread}.
"""
import contextlib

import torch

CONTROL, NAN_FILL, BIG_FILL = 0x00, 0xFF, 0x47
FILLS = (CONTROL, CONTROL, NAN_FILL, BIG_FILL)
_PATCHED = ("empty", "empty_like", "empty_strided")
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _fill_storage(t, byte):
    if not isinstance(t, torch.Tensor) or t.device.type == "meta" or t.is_sparse:
        return t
    st = t.untyped_storage()
    if st.nbytes() > 0:
        with torch.no_grad():
            torch.tensor([], dtype=torch.uint8, device=t.device).set_(st).fill_(byte)
    return t


@contextlib.contextmanager
def alloc_fill(byte):
    byte = int(byte)
    assert 0 <= byte <= 0xFF
    orig = {n: getattr(torch, n) for n in _PATCHED}
    orig_new_empty = torch.Tensor.new_empty

    def wrap(f):
        def filled(*args, **kwargs):
            return _fill_storage(f(*args, **kwargs), byte)
        filled.__name__ = getattr(f, "__name__", "filled")
        filled.__wrapped__ = f
        return filled

    try:
        for n, f in orig.items():
            setattr(torch, n, wrap(f))
        torch.Tensor.new_empty = wrap(orig_new_empty)
        yield
    finally:
        for n, f in orig.items():
            setattr(torch, n, f)
        torch.Tensor.new_empty = orig_new_empty


def _to_cpu(out):
    assert isinstance(out, dict) and out, "fn() returns a non-empty {name: tensor} dict"
    res = {}
    for k, v in out.items():
        v = v if isinstance(v, torch.Tensor) else torch.as_tensor(v)
        res[k] = v.detach().cpu().clone()
    return res


def run_under_fills(fn):
    """[control, control again, 0xFF, 0x47]: fn() under each fill; every result a {name: CPU tensor} dict."""
    results = []
    for byte in FILLS:
        with alloc_fill(byte):
            out = fn()
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            results.append(_to_cpu(out))        # (the copy to the host allocates too: still inside the fill)
    return results


def _bits(t):
    t = t.contiguous()
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    return t.view(_BITS[t.element_size()])


def _select(t, mask):
    return t if mask is None else t[mask]


def mismatches(results, masks=None):
    """-> ({name: reason} for every output that breaks the rule, {name: control-to-control spread})."""
    c0, c1, runs = results[0], results[1], {"0xFF": results[2], "0x47": results[3]}
    masks = masks or {}
    assert set(masks) <= set(c0), ("mask for an unknown output", set(masks) - set(c0))
    bad, spreads = {}, {}
    for k, a in c0.items():
        m = masks.get(k)
        if m is not None:
            m = m.cpu()
            assert m.dtype == torch.bool and m.shape == a.shape, (k, "mask shape")
            assert a.numel() == 0 or int((~m).sum()) * 2 < a.numel(), (k, "masked share must stay below one half")
        b = c1[k]
        assert b.shape == a.shape and b.dtype == a.dtype, (k, "control runs disagree in shape")
        exact = torch.equal(_bits(_select(a, m)), _bits(_select(b, m)))
        spread = 0.0
        if not exact:
            if not a.dtype.is_floating_point:
                bad[k] = "integer output differs between the two CONTROL runs"
                continue
            spread = float((_select(a, m).double() - _select(b, m).double()).abs().nan_to_num(nan=float("inf")).max())
        spreads[k] = spread
        for tag, r in runs.items():
            g = r.get(k)
            if g is None or g.shape != a.shape or g.dtype != a.dtype:
                bad[f"{k} [{tag}]"] = "missing, or another shape or dtype than the control"
                continue
            av, gv = _select(a, m), _select(g, m)
            if exact:
                if not torch.equal(_bits(av), _bits(gv)):
                    ne = _bits(av) != _bits(gv)
                    first = int(ne.reshape(-1).nonzero()[0]) if ne.numel() else -1
                    bad[f"{k} [{tag}]"] = (f"{int(ne.sum())} of {ne.numel()} elements differ from the control bitwise (controls agree bitwise); "
                                           f"first at flat index {first}: control {av.reshape(-1)[first].item()!r}, got {gv.reshape(-1)[first].item()!r}")
                continue
            ad, gd = av.double(), gv.double()
            scale = float(ad.abs().nan_to_num(nan=0.0, posinf=0.0, neginf=0.0).max()) if ad.numel() else 0.0
            bound = min(2.0 * spread, 1e-3 * scale)
            fresh_nonfinite = (~torch.isfinite(gd)) & torch.isfinite(ad)
            if bool(fresh_nonfinite.any()):
                bad[f"{k} [{tag}]"] = f"{int(fresh_nonfinite.sum())} NaN/Inf where the control has none (control spread {spread:.3g})"
                continue
            fin = torch.isfinite(ad)
            err = float((gd[fin] - ad[fin]).abs().max()) if bool(fin.any()) else 0.0
            if err > bound:
                bad[f"{k} [{tag}]"] = f"max |d| {err:.3g} > bound {bound:.3g} (control spread {spread:.3g}, largest entry {scale:.3g})"
    return bad, spreads


def assert_fill_independent(results, masks=None, tag=""):
    bad, spreads = mismatches(results, masks)
    nonzero = {k: v for k, v in spreads.items() if v != 0.0}
    assert not bad, (tag, "result depends on uninitialised memory", bad, "control-to-control spread", nonzero)
    return spreads
