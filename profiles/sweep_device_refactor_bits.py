#!/usr/bin/env python3
"""Same bits before and after a device-side refactor of the sweep kernels (one-off check; profiles/sweep_device_refactor_summary.txt,
profiles/sweep32_device_refactor_summary.txt and profiles/sweep64_device_refactor_summary.txt).

    QCOLLOC_HIP_VARIANT=parent python profiles/sweep_device_refactor_bits.py run DIR/parent.npz     # one fresh process per library
    python profiles/sweep_device_refactor_bits.py run DIR/new.npz
    python profiles/sweep_device_refactor_bits.py compare DIR/parent.npz DIR/new.npz                # on the CPU

`run` makes every call of the table below on host buffers and on device buffers, with all outputs together and with each output alone,
and saves every output array.  `run FILE PREFIX [host|dev]` keeps to the cases whose name starts with PREFIX and to one kind of buffer
(one fresh process per library and kind).  `compare` asserts with assert_array_equal that both sides hold the same arrays and counts
them; a side may be several files joined by commas (the host and the device run of one library).

    narrow ("mfma16-sweep")  N = 2, m = 2, p = 1, T = 6, free time, S in {3, 40}                       every entry point; stored-state grad, grad_params, vjp
                             the same with m = 8 (M = 8; the noise sweeps need m + p <= 8: not served)  every other entry point; stored-state walks
                             T = 8, S = 3, timesteps log-uniform: 0 .. 6 squarings in one call          every entry point; stored-state walks
    wide ("mfma32-sweep")    N = 9 (2N = 18: padded tiles), m = 1, p = 1, T = 4, S in {2, 20}           every entry point (wide = 1 + 2 + 16 + 64 + 256);
                                                                                                       stored-state grad, grad_params, vjp (wide = 1 + 2 + 8)
                             the same with m = 2                                                        the same
                             m = 1 with a fixed timestep (no timestep in the knot, nd = m)              the same
                             T = 8, S = 3, timesteps log-uniform: 0 .. 6 squarings in one call          the same
    64 ("mfma64-sweep")      N = 17 (2N = 34: padded tiles), 17 state columns (nct = 2), m = 1, p = 1,   every entry point but hvp (wide = 1 + 1024 + 2048 + 8192
                             T = 4, S in {2, 256}                                                       + 16384 + 65536); no stored-state walk in this form
                             the same with m = 2; with one ket column (nct = 1); with a fixed timestep  the same
                             m = 16, p = 8, S = 2: the widest part[] row, all 24 images                 the same
                             T = 8, S = 3, timesteps log-uniform: 0 .. 6 squarings in one call          the same
S = 2 and S = 3 give several chunks per sample, S = 20 and S = 40 a partly filled last workgroup, S = 256 one chunk per sample in the 64
form (its fill rule).  Asking for every output alone makes the
calls of the parameter flavours without `gs` as well.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NARROW = ("eval", "grad", "grad_params", "vjp", "jvp", "hvp", "noise_eval", "noise_grad")
REVERSE = ("grad", "grad_params", "vjp")
WIDE = dict(wide=True, wide_params=True, wide_tangent=True, wide_noise=True, wide_hessian=True)
WIDE_STORED = dict(wide=True, wide_params=True, stored_states=True, wide_stored=True)
WIDE64 = dict(wide=True, wide64=True, wide64_grad=True, wide64_params=True, wide64_tangent=True, wide64_noise=True)
ENTRIES64 = tuple(e for e in NARROW if e != "hvp")      # hvp refuses in this form
CASES = [dict(name="narrow", N=2, m=2, T=6, S=(3, 40), entries=NARROW, kw={}, stored=dict(stored_states=True), sq=None),
         dict(name="narrow-m8", N=2, m=8, T=6, S=(3,), entries=NARROW[:6], kw={}, stored=dict(stored_states=True), sq=None),
         dict(name="narrow-squarings", N=2, m=2, T=8, S=(3,), entries=NARROW, kw={}, stored=dict(stored_states=True), sq=7),
         dict(name="wide", N=9, m=1, T=4, S=(2, 20), entries=NARROW, kw=WIDE, stored=WIDE_STORED, sq=None),
         dict(name="wide-m2", N=9, m=2, T=4, S=(2, 20), entries=NARROW, kw=WIDE, stored=WIDE_STORED, sq=None),
         dict(name="wide-fixed-dt", N=9, m=1, T=4, S=(2, 20), entries=NARROW, kw=dict(WIDE, dt_fixed=0.2), stored=dict(WIDE_STORED, dt_fixed=0.2),
              sq=None),
         dict(name="wide-squarings", N=9, m=1, T=8, S=(3,), entries=NARROW, kw=WIDE, stored=WIDE_STORED, sq=7),
         dict(name="64", N=17, m=1, T=4, S=(2, 256), entries=ENTRIES64, kw=WIDE64, stored=None, sq=None),
         dict(name="64-m2", N=17, m=2, T=4, S=(2, 256), entries=ENTRIES64, kw=WIDE64, stored=None, sq=None),
         dict(name="64-ket", N=17, m=1, T=4, S=(2, 256), entries=ENTRIES64, kw=WIDE64, stored=None, sq=None, ket=True),
         dict(name="64-fixed-dt", N=17, m=1, T=4, S=(2, 256), entries=ENTRIES64, kw=dict(WIDE64, dt_fixed=0.2), stored=None, sq=None),
         dict(name="64-m16-p8", N=17, m=16, p=8, T=4, S=(2,), entries=ENTRIES64, kw=WIDE64, stored=None, sq=None),
         dict(name="64-squarings", N=17, m=1, T=8, S=(3,), entries=ENTRIES64, kw=WIDE64, stored=None, sq=7)]


def run(path, prefix="", where=("host", "dev")):
    import torch

    import __graft_entry__ as g
    import sweep_reference as ref
    import test_sweep as ts
    from test_sweep_shared_staging import ENTRIES
    qc = g.load_package()
    L = qc._lib
    print("library:", L.LIB_PATH, flush=True)
    saved = {}

    def call(sw, entry, Z, init, S, data, sizes, want, device):
        ins, outs = ENTRIES[entry]
        given = [np.ascontiguousarray(data[name], dtype=np.float64) for name in ins]
        if device:
            dev = lambda a: torch.from_numpy(a).cuda()
            dZ, dinit, din = dev(Z), dev(init), [dev(a) for a in given]
            dout = {o: torch.full((sizes[o],), float("nan"), dtype=torch.float64, device="cuda") for o in want}
            ptr = lambda t: None if t is None else t.data_ptr()
            rc = getattr(L.lib, f"qc_sweep_{entry}_dev")(sw._h, ptr(dZ), ptr(dinit), S, *[ptr(t) for t in din], *[ptr(dout.get(o)) for o in outs],
                                                         torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res = {o: t.cpu().numpy() for o, t in dout.items()}
        else:
            res = {o: np.full(sizes[o], np.nan) for o in want}
            rc = getattr(L.lib, f"qc_sweep_{entry}")(sw._h, L.dptr(Z), L.dptr(init), S, *[L.dptr(a) for a in given],
                                                     *[None if o not in res else L.dptr(res[o]) for o in outs])
        assert rc == L.QC_OK, (entry, want, L.lib.qc_sweep_last_error(sw._h).decode())
        return res

    for c in CASES:
        if not c["name"].startswith(prefix):
            continue
        N, m, T, p = c["N"], c["m"], c["T"], c.get("p", 1)
        rng = np.random.default_rng(len(c["name"]) + 100 * m)
        H0, Hd, Pm = ts._herm(rng, N), [ts._herm(rng, N, 0.4) for _ in range(m)], ts._herm(rng, N)
        Ps = [Pm] + [ts._herm(rng, N) for _ in range(p - 1)]
        goal, init = qc.operator_to_iso_vec(ts._unitary(rng, N)), qc.operator_to_iso_vec(ts._unitary(rng, N))
        state = dict(goal=goal, fid_kind="unitary")
        if c.get("ket"):      # one column: the first of each unitary, (re, im)
            ket = lambda U: np.concatenate([U[:, 0].real, U[:, 0].imag])
            goal, init = ket(ts._unitary(rng, N)), ket(ts._unitary(rng, N))
            state = dict(goal=goal, fid_kind="ket", cols=1)
        controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
        per_S = {S: dict(theta=rng.uniform(-0.3, 0.3, (S, p)), scale=rng.uniform(0.9, 1.1, (S, m)), weights=rng.uniform(0.5, 1.5, S))
                 for S in c["S"]}
        if c["sq"]:      # interval t of sample 0 needs exactly t squarings (the way tests/test_sweep_grad.py scales its systems)
            G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(H) for H in Ps]
            d0 = per_S[c["S"][0]]
            norm = lambda s, t: np.abs(ref.sample_generator(G0, Gd, Gp, controls[:, t], d0["theta"][s], d0["scale"][s])).sum(axis=0).max()
            dts = np.array([0.09 * 2.0 ** t / norm(0, t) for t in range(T - 1)] + [0.1])
            seen = {ts._squarings(dts[t] * norm(s, t)) for s in range(c["S"][0]) for t in range(T - 1)}
            assert set(range(c["sq"])) <= seen, seen
            print(f"{c['name']}: squarings of the call {sorted(seen)}", flush=True)
        system = qc.QuantumSystem(H0, Hd)
        for kind, kw, entries in (("closed", c["kw"], c["entries"]), ("stored", c["stored"], REVERSE)):
            if kw is None:
                continue
            sw = qc.RolloutSweep(system, Ps, T, **state, **kw)
            ns, Zlen, nd = sw.ns, sw.Z_len, sw.n_deriv
            Z = sw.pack(controls, dts)
            vrng = np.random.default_rng(7)
            for S in c["S"]:
                data = dict(per_S[S], cot=vrng.standard_normal((S, ns)), vZ=vrng.standard_normal(Zlen), vinit=vrng.standard_normal(ns),
                            vtheta=vrng.standard_normal((S, p)), vscale=vrng.standard_normal((S, m)), vcot=vrng.standard_normal((S, ns)),
                            noise=vrng.uniform(-0.3, 0.3, (S, T - 1, p)))
                sizes = dict(finals=S * ns, fids=S, tfinals=S * ns, tfids=S, J=1, grad=Zlen, gs=S * (T - 1) * nd, ginit=S * ns, gth=S * p,
                             gsc=S * m, tgrad=Zlen, tgs=S * (T - 1) * nd, tginit=S * ns, gn=S * (T - 1) * p)
                for entry in entries:
                    outs = ENTRIES[entry][1]
                    for device in [d for d in (False, True) if ("dev" if d else "host") in where]:
                        for want in (outs,) + tuple((o,) for o in outs):
                            res = call(sw, entry, Z, init, S, data, sizes, want, device)
                            for o, a in res.items():
                                assert np.isfinite(a).all(), (c["name"], kind, entry, S, want, o)
                                saved[f"{c['name']}|{kind}|{sw.kernel_name}|S={S}|{entry}|{'dev' if device else 'host'}|{'+'.join(want)}|{o}"] = a
            print(f"{c['name']} {kind}: {sw.kernel_name}, launches {[sw.launch(S) for S in c['S']]}, {len(saved)} arrays so far", flush=True)
            sw.close()
    np.savez(path, **saved)
    print(f"saved {len(saved)} arrays, {sum(a.size for a in saved.values())} values to {path}")


def compare(pa, pb):
    load = lambda paths: {k: a for path in paths.split(",") for k, a in np.load(path).items()}
    A, B = load(pa), load(pb)
    assert sorted(A) == sorted(B), "the two runs saved different sets of arrays"
    values = 0
    for k in A:
        np.testing.assert_array_equal(A[k], B[k], err_msg=k)
        values += A[k].size
    # within one side: an output asked for alone carries the bits of the same output asked for with the others, host and device
    alone = 0
    for k in A:
        case, kind, form, S, entry, where, want, o = k.split("|")
        if "+" not in want and where == "host":
            twins = [q for q in A if q.split("|")[:5] == [case, kind, form, S, entry] and q.split("|")[7] == o]
            for q in twins:
                np.testing.assert_array_equal(B[q], B[k], err_msg=f"{q} against {k}")
                alone += 1
    print(f"BITS: {len(A)} arrays compared with assert_array_equal, all equal; {values} values "
          f"({alone} comparisons of one output across host / device and alone / together inside the new file, all equal)")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], *sys.argv[3:4], *[(w,) for w in sys.argv[4:5]])
    else:
        compare(sys.argv[2], sys.argv[3])
