"""One long-lived sweep handle, every host-buffer entry point interleaved: the staging buffers of a handle are shared between its entry
points (finals: eval, vjp, jvp, noise_eval; fids: eval, grad, jvp, noise_eval, noise_grad; theta, scale: all; per-sample gradients and the
dense gradient: grad, vjp, noise_grad; grad_theta, grad_scale: grad_params, vjp; the cotangent: vjp, hvp; the directions: jvp, hvp), each
follows the largest request so far, and every entry point asks for its own size.  A buffer that one entry
point sized for another, or that two of them should not share, shows as a result that differs from the same call on a fresh handle.
S alternates small, large, small and every call asks for a different subset of outputs; the sequence then runs once more through the
`_dev` entry points (their scratch is shared likewise: chunk totals, chunk-end states and adjoints, per-interval derivatives).
Every array must equal, bit for bit, the same call on a handle created for it.  The other sweep tests grow one entry point's buffers at a time.
Hessian products and noise sweeps came after the first 14 steps and follow them: they use dTot, dXs, dLs, dGfid and dGsamp of the entries
before them next to buffers of their own (dXsT, dLsT, dTGsamp; the staged noise and its gradient), so each of their steps is followed by
the older entry that reads the same scratch -- `vjp` after `hvp`, `grad` after `noise_grad`, `eval` after `noise_eval`.

Shapes: "mfma16-sweep" N = 2, two drives, one perturbation, T = 6, free timestep, S = 3 (three chunks) and 40; "mfma32-sweep" N = 9 wide,
one drive, T = 4, S = 2 and 20 (no pushforward, no parameter gradients, no Hessian products and no noise sweeps in that form: those steps
are left out there, and the form runs the first 14 steps as it always did)."""
import numpy as np
import pytest
import torch

import test_sweep as ts

FORMS = {"mfma16-sweep": dict(N=2, m=2, p=1, T=6, wide=False, S=(3, 40)),
         "mfma32-sweep": dict(N=9, m=1, p=1, T=4, wide=True, S=(2, 20))}

# entry point -> (inputs after S, outputs) in the order of the C prototype
ENTRIES = {"eval": (("theta", "scale"), ("finals", "fids")),
           "grad": (("theta", "scale", "weights"), ("fids", "J", "grad", "gs")),
           "grad_params": (("theta", "scale", "weights"), ("fids", "J", "grad", "gs", "gth", "gsc")),
           "vjp": (("theta", "scale", "cot"), ("finals", "grad", "gs", "ginit", "gth", "gsc")),
           "jvp": (("theta", "scale", "vZ", "vinit", "vtheta", "vscale"), ("finals", "fids", "tfinals", "tfids")),
           "hvp": (("theta", "scale", "cot", "vZ", "vinit", "vtheta", "vscale", "vcot"), ("tgrad", "tgs", "tginit")),
           "noise_eval": (("theta", "scale", "noise"), ("finals", "fids")),
           "noise_grad": (("theta", "scale", "noise", "weights"), ("fids", "J", "grad", "gs", "gn"))}
NEW = ("hvp", "noise_eval", "noise_grad")        # "mfma16-sweep" handles only
FOLLOWED_BY = {"hvp": "vjp", "noise_grad": "grad", "noise_eval": "eval"}      # the older entry that reads the same scratch

# (entry point, 0 = small S / 1 = large S, outputs asked for, inputs left out)
SEQUENCE = [("eval", 0, ("finals", "fids"), ()),
            ("vjp", 1, ("gs", "ginit", "gth", "gsc"), ()),
            ("jvp", 0, ("fids", "tfinals", "tfids"), ()),
            ("grad", 1, ("fids", "gs"), ()),
            ("grad_params", 0, ("J", "grad", "gth", "gsc"), ()),
            ("eval", 1, ("fids",), ()),
            ("vjp", 0, ("finals",), ("scale",)),
            ("jvp", 1, ("finals", "tfids"), ("vinit", "vtheta", "vscale")),
            ("grad", 0, ("J", "grad"), ("weights",)),
            ("vjp", 1, ("finals", "grad"), ()),
            ("grad_params", 1, ("fids", "gs", "gth"), ("scale",)),
            ("jvp", 0, ("tfinals",), ("vZ",)),
            ("eval", 0, ("finals",), ()),
            ("grad", 1, ("fids", "J", "grad", "gs"), ()),
            # Hessian products and noise sweeps, each followed by the older entry that reads the same scratch
            ("hvp", 0, ("tgrad", "tgs", "tginit"), ()),
            ("vjp", 1, ("grad", "gs", "ginit"), ()),
            ("noise_grad", 0, ("fids", "J", "grad", "gn"), ()),
            ("grad", 1, ("J", "grad"), ("weights",)),
            ("noise_eval", 1, ("finals", "fids"), ()),
            ("eval", 0, ("finals", "fids"), ()),
            ("hvp", 1, ("tgs",), ("vinit", "vtheta", "vscale", "vcot")),
            ("vjp", 0, ("gs", "gth"), ("scale",)),
            ("noise_grad", 1, ("fids", "gs", "gn"), ("weights", "scale")),
            ("grad", 0, ("fids", "gs"), ()),
            ("noise_eval", 0, ("fids",), ("scale",)),
            ("eval", 1, ("finals",), ()),
            ("hvp", 0, ("tgrad", "tginit"), ("vZ",)),
            ("vjp", 1, ("finals", "gs"), ()),
            ("noise_grad", 0, ("J", "grad", "gs"), ()),
            ("grad", 1, ("fids", "J", "grad", "gs"), ())]
N_BASE = 14        # the steps from before Hessian products and noise sweeps: the prefix, unchanged


def steps_of(form):
    """The sequence as a form serves it: wide handles have no pushforward, no parameter gradients and no parameter cotangents, and
    neither Hessian products nor noise sweeps: they run the first `N_BASE` steps."""
    if not FORMS[form]["wide"]:
        return SEQUENCE
    out = []
    for entry, k, want, drop in SEQUENCE[:N_BASE]:
        want = tuple(w for w in want if w not in ("gth", "gsc"))
        if entry not in ("jvp", "grad_params") + NEW and want:
            out.append((entry, k, want, drop))
    return out


def test_sequences_cover_the_shared_buffers():
    """Every entry point of a form occurs at both sizes or after a call of the other size, and every shared output is asked for by
    each entry point that has it, on the form that serves it."""
    for form, f in FORMS.items():
        steps = steps_of(form)
        entries = {e for e, *_ in steps}
        assert entries == ({"eval", "grad", "vjp"} if f["wide"] else set(ENTRIES))
        for shared in ("finals", "fids", "grad", "gs") + (() if f["wide"] else ("gth", "gsc")):
            users = {e for e, (_, outs) in ENTRIES.items() if shared in outs and e in entries}
            assert users == {e for e, _, want, _ in steps if shared in want}, (form, shared)
        sizes = [k for _, k, _, _ in steps]
        assert 0 in sizes and 1 in sizes and sizes[0] == 0 and any(a == 1 and b == 0 for a, b in zip(sizes, sizes[1:]))
    # the steps from before Hessian products and noise sweeps are the prefix, as they were
    assert len(SEQUENCE) > N_BASE == 14 and not any(e in NEW for e, *_ in SEQUENCE[:N_BASE])
    assert SEQUENCE[0] == ("eval", 0, ("finals", "fids"), ()) and SEQUENCE[N_BASE - 1] == ("grad", 1, ("fids", "J", "grad", "gs"), ())
    assert [e for e, *_ in SEQUENCE[:N_BASE]] == ["eval", "vjp", "jvp", "grad", "grad_params", "eval", "vjp", "jvp", "grad", "vjp", "grad_params", "jvp",
                                                  "eval", "grad"]
    assert all(e in ("eval", "grad", "vjp") for e, *_ in steps_of("mfma32-sweep")) and len(steps_of("mfma32-sweep")) == 9
    tail = SEQUENCE[N_BASE:]
    for entry in NEW:
        mine = [(i, k, want) for i, (e, k, want, _) in enumerate(tail) if e == entry]
        ks = [k for _, k, _ in mine]
        assert {0, 1} <= set(ks) and any(a == 1 and b == 0 for a, b in zip(ks, ks[1:])), entry      # both sizes, large and then small
        asked = {w for _, _, want in mine for w in want}
        assert asked == set(ENTRIES[entry][1]), (entry, asked)                                      # every output at least once
        # each step sits between calls of the older entries: one before it, and right after it the one that reads the same scratch, at the other size
        for i, k, _ in mine:
            assert tail[i + 1][0] == FOLLOWED_BY[entry] and tail[i + 1][1] != k, (entry, i)
            assert SEQUENCE[N_BASE + i - 1][0] not in NEW, (entry, i)
    assert {"tgrad", "tgs", "tginit"} == set(ENTRIES["hvp"][1]) and "gn" in ENTRIES["noise_grad"][1]
    # the handle's own per-sample buffers take the place of an output that is not asked for, at least once per entry
    assert any(e == "noise_grad" and "grad" in want and "gs" not in want for e, _, want, _ in tail)
    assert any(e == "hvp" and "tgrad" in want and "tgs" not in want for e, _, want, _ in tail)
    # a Hessian product keeps a direction and a noise sweep its noise, whatever else is left out
    dirs = ("vZ", "vinit", "vtheta", "vscale", "vcot")
    for e, _, _, drop in tail:
        assert "cot" not in drop and "noise" not in drop and "theta" not in drop
        assert e != "hvp" or set(dirs) - set(drop)


class Problem:
    def __init__(self, qc, form):
        f = FORMS[form]
        rng = np.random.default_rng(len(form))
        N, m, p, T = f["N"], f["m"], f["p"], f["T"]
        self.f, self.qc = f, qc
        self.system = qc.QuantumSystem(ts._herm(rng, N), [ts._herm(rng, N, 0.4) for _ in range(m)])
        self.perts = [ts._herm(rng, N) for _ in range(p)]
        self.goal = qc.operator_to_iso_vec(ts._unitary(rng, N))
        sw = self.handle()
        self.ns, self.Zlen, self.nd = sw.ns, sw.Z_len, sw.n_deriv
        self.Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
        sw.close()
        self.init = qc.operator_to_iso_vec(ts._unitary(rng, N))
        self.shared = dict(vZ=rng.standard_normal(self.Zlen), vinit=rng.standard_normal(self.ns))
        self.per_S = [dict(theta=rng.uniform(-0.3, 0.3, (S, p)), scale=rng.uniform(0.9, 1.1, (S, m)), weights=rng.uniform(0.5, 1.5, S),
                           cot=rng.standard_normal((S, self.ns)), vtheta=rng.standard_normal((S, p)), vscale=rng.standard_normal((S, m)))
                      for S in f["S"]]
        for S, d in zip(f["S"], self.per_S):      # drawn after everything above: the inputs of the first 14 steps are what they were
            d.update(vcot=rng.standard_normal((S, self.ns)), noise=rng.uniform(-0.3, 0.3, (S, T - 1, p)))

    def handle(self):
        f = self.f
        return self.qc.RolloutSweep(self.system, self.perts, f["T"], goal=self.goal, fid_kind="unitary", wide=f["wide"])

    def sizes(self, S):
        f = self.f
        return dict(finals=S * self.ns, fids=S, tfinals=S * self.ns, tfids=S, J=1, grad=self.Zlen, gs=S * (f["T"] - 1) * self.nd, ginit=S * self.ns,
                    gth=S * f["p"], gsc=S * f["m"], tgrad=self.Zlen, tgs=S * (f["T"] - 1) * self.nd, tginit=S * self.ns, gn=S * (f["T"] - 1) * f["p"])

    def call(self, sw, step, device):
        """The raw library call of one step on host buffers or on device tensors: {output name: numpy array}."""
        L = self.qc._lib
        entry, k, want, drop = step
        S, data = self.f["S"][k], dict(self.shared, **self.per_S[k])
        ins, outs = ENTRIES[entry]
        given = [None if name in drop else np.ascontiguousarray(data[name]) for name in ins]
        sizes = self.sizes(S)
        if device:
            dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
            dZ, dinit, din = dev(self.Z), dev(self.init), [dev(a) for a in given]
            dout = {o: torch.full((sizes[o],), float("nan"), dtype=torch.float64, device="cuda") for o in want}
            ptr = lambda t: None if t is None else t.data_ptr()
            rc = getattr(L.lib, f"qc_sweep_{entry}_dev")(sw._h, ptr(dZ), ptr(dinit), S, *[ptr(t) for t in din], *[ptr(dout.get(o)) for o in outs],
                                                         torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res = {o: t.cpu().numpy() for o, t in dout.items()}
        else:
            opt = lambda a: None if a is None else L.dptr(a)
            res = {o: np.full(sizes[o], np.nan) for o in want}
            rc = getattr(L.lib, f"qc_sweep_{entry}")(sw._h, L.dptr(self.Z), L.dptr(self.init), S, *[opt(a) for a in given],
                                                     *[opt(res.get(o)) for o in outs])
        assert rc == L.QC_OK, (step, L.lib.qc_sweep_last_error(sw._h).decode())
        return res


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_interleaved_calls_on_one_handle_match_fresh_handles(qc, form):
    prob = Problem(qc, form)
    steps = steps_of(form)
    kept = prob.handle()
    try:
        assert kept.kernel_name == form and kept.launch(FORMS[form]["S"][0])[2] > 1      # the small S splits the trajectory into chunks
        for device in (False, True):
            for i, step in enumerate(steps):
                got = prob.call(kept, step, device)
                fresh = prob.handle()
                try:
                    want = prob.call(fresh, step, device)
                finally:
                    fresh.close()
                assert set(got) == set(step[2])
                for name in step[2]:
                    assert np.isfinite(want[name]).all(), (i, step, name)
                    np.testing.assert_array_equal(got[name], want[name], err_msg=f"step {i} {step} {'device' if device else 'host'}: {name}")
    finally:
        kept.close()
