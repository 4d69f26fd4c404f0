"""Every kernel of a sweep form forms the same generator and chooses the same number of squarings: the shared device headers
(qc_sweep_common.h, qc_sweep16_common.h, qc_sweep32_common.h) carry that rule once.  What follows from it, held together in one call
whose intervals need 0 up to at least 4 squarings (timesteps spread log-uniformly: interval t of sample 0 has ||dt_t G||_1 = 0.09 x 2^t)
and whose launch has more than one chunk:

    finals  of qc_sweep_eval, qc_sweep_vjp and qc_sweep_jvp are the same bits;
    fids    of qc_sweep_eval, qc_sweep_grad, qc_sweep_jvp and of qc_sweep_grad on a twin handle that walks stored states are the same bits.

The documentation promises each relation and single tests assert most of them one at a time, at one or two squarings.
Shapes: "mfma16-sweep" N = 2, two drives, one perturbation; "mfma32-sweep" N = 9, one drive (wide: the handle of eval, vjp, jvp and grad
carries the tangent bit only, the stored bits are on the twin, which carries both); T = 8, S = 3, free timesteps."""
import numpy as np
import pytest

import sweep_reference as ref
import test_sweep as ts
from test_sweep_shared_staging import ENTRIES

FORMS = {"mfma16-sweep": dict(N=2, m=2, wide={}, twin=dict(stored_states=True)),
         "mfma32-sweep": dict(N=9, m=1, wide=dict(wide=True, wide_tangent=True),
                              twin=dict(wide=True, wide_tangent=True, stored_states=True, wide_stored=True))}
T, S, P = 8, 3, 1


def raw_call(qc, sw, entry, Z, init, S, given, want):
    """One host-buffer library call: `given` {input name: array} (a missing one is NULL), `want` the outputs asked for with their sizes.
    Returns {output name: array}."""
    L = qc._lib
    ins, outs = ENTRIES[entry]
    opt = lambda a: None if a is None else L.dptr(a)
    held = [None if given.get(name) is None else np.ascontiguousarray(given[name], dtype=np.float64) for name in ins]
    res = {o: np.full(n, np.nan) for o, n in want.items()}
    rc = getattr(L.lib, f"qc_sweep_{entry}")(sw._h, L.dptr(Z), L.dptr(init), S, *[opt(a) for a in held], *[opt(res.get(o)) for o in outs])
    assert rc == L.QC_OK, (entry, L.lib.qc_sweep_last_error(sw._h).decode())
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_every_kernel_takes_the_forward_sweeps_squarings(qc, form):
    f = FORMS[form]
    N, m = f["N"], f["m"]
    rng = np.random.default_rng(len(form))
    H0, Hd, Pm = ts._herm(rng, N), [ts._herm(rng, N, 0.4) for _ in range(m)], ts._herm(rng, N)
    goal, init = qc.operator_to_iso_vec(ts._unitary(rng, N)), qc.operator_to_iso_vec(ts._unitary(rng, N))
    controls = rng.uniform(-1, 1, (m, T))
    theta, scale = rng.uniform(-0.3, 0.3, (S, P)), rng.uniform(0.9, 1.1, (S, m))
    G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(Pm)]
    norm = lambda s, t: np.abs(ref.sample_generator(G0, Gd, Gp, controls[:, t], theta[s], scale[s])).sum(axis=0).max()
    # interval t of sample 0 needs exactly t squarings; the last knot's timestep is not read
    dts = np.array([0.09 * 2.0 ** t / norm(0, t) for t in range(T - 1)] + [0.1])
    seen = {ts._squarings(dts[t] * norm(s, t)) for s in range(S) for t in range(T - 1)}
    assert set(range(5)) <= seen, seen

    system = qc.QuantumSystem(H0, Hd)
    sw = qc.RolloutSweep(system, [Pm], T, goal=goal, fid_kind="unitary", **f["wide"])
    twin = qc.RolloutSweep(system, [Pm], T, goal=goal, fid_kind="unitary", **f["twin"])
    try:
        assert sw.kernel_name == form and twin.kernel_name == form and sw.launch(S)[2] > 1
        Z, ns = sw.pack(controls, dts), sw.ns
        data = dict(theta=theta, scale=scale, cot=rng.standard_normal((S, ns)), vZ=rng.standard_normal(sw.Z_len))
        call = lambda h, entry, want: raw_call(qc, h, entry, Z, init, S, data, want)
        ev = call(sw, "eval", dict(finals=S * ns, fids=S))
        vj = call(sw, "vjp", dict(finals=S * ns, grad=sw.Z_len))
        jv = call(sw, "jvp", dict(finals=S * ns, fids=S, tfinals=S * ns))
        gr = call(sw, "grad", dict(fids=S, grad=sw.Z_len))
        st = call(twin, "grad", dict(fids=S, grad=sw.Z_len))
        assert np.isfinite(ev["finals"]).all() and np.isfinite(ev["fids"]).all()
        np.testing.assert_array_equal(vj["finals"], ev["finals"], err_msg="finals: vjp against eval")
        np.testing.assert_array_equal(jv["finals"], ev["finals"], err_msg="finals: jvp against eval")
        np.testing.assert_array_equal(gr["fids"], ev["fids"], err_msg="fids: grad against eval")
        np.testing.assert_array_equal(jv["fids"], ev["fids"], err_msg="fids: jvp against eval")
        np.testing.assert_array_equal(st["fids"], ev["fids"], err_msg="fids: stored-state grad (twin handle) against eval")
    finally:
        sw.close()
        twin.close()
