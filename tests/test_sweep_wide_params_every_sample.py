"""Parameter gradients and parameter cotangents on wide handles (`wide=True, wide_params=True`, "mfma32-sweep") at mid-size and filled
launches, EVERY sample against the CPU reference: the method of tests/test_sweep_every_sample.py (read its header) for the parameter
flavour of the wide walk, which runs TWO waves a workgroup (item = 2 blockIdx + wave) where every other walk runs four.  A launch of S
samples is made of R = 8 distinct parameter rows; sample s carries row cls[s]; the forward-mode references are computed once for the R
rows; every output row is compared with its row's reference at the tolerance the output has in its own test file, and carries the bits
of the first sample of its class.  S = 301 (several chunks, an odd item count) and S = 2049 (one chunk, past the fill threshold); one
handle grown from 301 to 2049 and reused at 97 against fresh handles.  No tolerance is new.
Measured worst ratios: profiles/sweep_wide_param_summary.txt."""
import numpy as np
import pytest

import test_sweep as ts
import test_sweep_every_sample as tes
import test_sweep_grad as tg
import test_sweep_param_grad as tp
import test_sweep_vjp as tv
import test_sweep_wide as tw

R = tes.R
LEVELS, M, P, T = 9, 2, 1, 11
GROWTH = (301, 2049, 97)
_ROWS = {}


def rows_of(qc):
    """The R distinct rows as a case of their own (what the references are computed for): built once, shared, never written to."""
    if "rows" not in _ROWS:
        rows = tw.build(qc, "every/wide-params", ("unitary", LEVELS, M, P, True, True, R, T, ("unitary", [0, 1, 3, 4], "abs"), None))
        rows["cot"] = tv.unit_cotangents(np.random.default_rng(11), R, rows["init"].size)
        _ROWS["rows"] = rows
    return _ROWS["rows"]


def make(qc, rows):
    return ts.make_sweep(qc, rows, wide=True, wide_params=True)


def assert_launch(sw, S):
    want = tw.wide_launch(2 * LEVELS, M, S, T)
    assert sw.kernel_name == "mfma32-sweep" and sw.launch(S) == (True, want["chunk"], want["n_chunks"])
    return want


def check_params(qc, sw, rows, c, what):
    """`qc_sweep_grad_params` with every output (buffers prefilled with -7), then `param_grad` as callers use it."""
    cls = c["cls"]
    Z = sw.pack(c["controls"], c["dts"])
    o = tp._raw(qc, sw, Z, c["init"], c["theta"], c["scale"], c["weights"])
    tp._assert_params(o["gth"], o["gsc"], tes.params_case(rows, c), what)
    tes.every_sample(tg._assert_samples, o["gs"], tes.ref_grad(rows)[cls], cls, what)
    for k in ("gth", "gsc", "gs"):
        tes.assert_class_bits(o[k], cls, f"{what} {k}")
    tes.assert_fidelities(o["fids"], o["J"], rows, c, what)
    tes.assert_dense(o["grad"], tes.ref_grad(rows), cls, c["weights"], sw, tg.GRAD_RTOL, what)
    fids, gth, gsc = sw.param_grad(Z, c["init"], c["theta"], c["scale"])
    for a, k in ((fids, "fids"), (gth, "gth"), (gsc, "gsc")):
        np.testing.assert_array_equal(a, o[k], err_msg=k)
    return o


def check_vjp_params(sw, rows, c, what, form="32"):
    """One `vjp_device` call with every output, the parameter cotangents among them.  `form`: the key of `tv.reference`'s cache."""
    cls = c["cls"]
    Z = sw.pack(c["controls"], c["dts"])
    out = tv.device_call(sw, Z, c, list(tv.OUTPUTS))
    r = tv.reference(rows, form)
    for k in ("grad_samples", "grad_theta", "grad_scale"):
        tes.every_sample(tv.assert_samples, out[k], r[k][cls], cls, f"{what} {k}")
    tes.every_sample(tv.assert_init, out["grad_init"], r["grad_init"][cls], cls, f"{what} grad_init")
    for k in tv.OUTPUTS:
        if k != "grad":
            tes.assert_class_bits(out[k], cls, f"{what} {k}")
    tes.assert_dense(out["grad"], r["grad_samples"], cls, np.ones(c["S"]), sw, tv.VJP_RTOL, what)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("S", [301, 2049])
def test_wide_param_grad_every_sample(qc, S):
    rows = rows_of(qc)
    c = tes.expand(rows, S)
    sw = make(qc, rows)
    try:
        want = assert_launch(sw, S)
        assert (want["n_chunks"], S * want["n_chunks"] % 2) == ((1, 1) if S == 2049 else (4, 0))      # S = 2049: the last workgroup holds one wave
        check_params(qc, sw, rows, c, f"32/every/wide-params S = {S}")
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_vjp_params_every_sample(qc):
    rows = rows_of(qc)
    c = tes.expand(rows, 301)
    sw = make(qc, rows)
    try:
        assert_launch(sw, 301)
        check_vjp_params(sw, rows, c, "32/every/wide-params pullback S = 301")
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_params_scratch_growth_every_sample(qc):
    """One handle at S = 301, then 2049, then 97: dPart, dXs, dLs and dGsamp grow and are then reused at a smaller stride.  At every S
    the outputs of `qc_sweep_grad_params` and of the pullback carry the bits of a fresh handle's and pass the checks above."""
    rows = rows_of(qc)
    sw = make(qc, rows)
    try:
        seen = []
        for S in GROWTH:
            c = tes.expand(rows, S)
            seen.append(assert_launch(sw, S)["n_chunks"])
            what = f"32/every/wide-params grown to S = {S}"
            o = check_params(qc, sw, rows, c, what)
            out = check_vjp_params(sw, rows, c, what + " pullback") if S != 2049 else None
            fresh = make(qc, rows)
            try:
                Z = fresh.pack(c["controls"], c["dts"])
                o2 = tp._raw(qc, fresh, Z, c["init"], c["theta"], c["scale"], c["weights"])
                out2 = tv.device_call(fresh, Z, c, list(out)) if out is not None else None
            finally:
                fresh.close()
            assert o["J"] == o2["J"]
            for k in ("fids", "grad", "gs", "gth", "gsc"):
                np.testing.assert_array_equal(o[k], o2[k], err_msg=f"S = {S}: {k}")
            if out is not None:
                for k in out:
                    np.testing.assert_array_equal(out[k], out2[k], err_msg=f"S = {S}: pullback {k}")
        assert seen[1] == 1 and seen[0] > 1 and seen[2] > 1 and GROWTH[1] * seen[1] > GROWTH[2] * seen[2]
    finally:
        sw.close()
