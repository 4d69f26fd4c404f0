"""What the Python binding of the rollout sweeps sends to the library, pinned call by call (no GPU: the library is replaced by a
recording stand-in).

Every public entry of `RolloutSweep` is called on three small handles -- once with every optional argument given, once with each one left
out in turn -- and every refusal (ValueError) of the class and of the three one-shot functions is provoked by a single-fault input.  For
every evaluation symbol the stand-in records its name, S, which pointer arguments are null and, for host inputs, the values behind the
pointer (read for the length include/qcolloc.h documents).  The recorded calls, the shapes and types of what comes back and the types and
messages of what is raised are compared with tests/golden/sweep_binding_calls.json.

The golden file is recorded results: `QC_RECORD_SWEEP_BINDING_CALLS=1 pytest tests/test_sweep_binding_calls.py` writes it, and it was
written that way with the rollouts.py / objectives.py / _lib.py of the commit BEFORE the binding was consolidated ("one argument check and
one call path for all entries"), so it pins what the copied-out entries sent.  The test reaches the binding through public names and
`_lib.lib` alone, so it runs unchanged against either revision of those three files.
"""
import inspect
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_binding_calls.json")
RECORDING = bool(os.environ.get("QC_RECORD_SWEEP_BINDING_CALLS"))
S = 2

# the arguments of the sixteen evaluation symbols after the handle (include/qcolloc.h); the device forms end with the stream
_COMMON = ("Z", "init", "S", "theta", "scale")
SYMBOL_ARGS = {
    "qc_sweep_eval": _COMMON + ("finals", "fids"),
    "qc_sweep_grad": _COMMON + ("weights", "fids", "J", "grad", "grad_samples"),
    "qc_sweep_grad_params": _COMMON + ("weights", "fids", "J", "grad", "grad_samples", "grad_theta", "grad_scale"),
    "qc_sweep_vjp": _COMMON + ("cot", "finals", "grad", "grad_samples", "grad_init", "grad_theta", "grad_scale"),
    "qc_sweep_jvp": _COMMON + ("vZ", "vinit", "vtheta", "vscale", "finals", "fids", "tfinals", "tfids"),
    "qc_sweep_hvp": _COMMON + ("cot", "vZ", "vinit", "vtheta", "vscale", "vcot", "tgrad", "tgrad_samples", "tgrad_init"),
    "qc_sweep_noise_eval": _COMMON + ("noise", "finals", "fids"),
    "qc_sweep_noise_grad": _COMMON + ("noise", "weights", "fids", "J", "grad", "grad_samples", "grad_noise"),
}
SYMBOL_ARGS.update({name + "_dev": args + ("stream",) for name, args in list(SYMBOL_ARGS.items())})
PASS_THROUGH = {"qc_sweep_desc_launch"} | {f"qc_sweep_desc_{e}_supported" for e in ("grad", "vjp", "jvp", "hvp", "noise")}


def input_lengths(d, S):
    """The documented length of every host INPUT of the evaluation symbols, from the descriptor the handle was made with."""
    ns = 2 * d["N"] * (d["state_cols"] or d["N"])
    Z_len = d["T"] * d["zdim"] + d["global_dim"]
    return {"Z": Z_len, "init": ns, "theta": S * d["n_pert"], "scale": S * d["m"], "weights": S, "cot": S * ns, "vZ": Z_len, "vinit": ns,
            "vtheta": S * d["n_pert"], "vscale": S * d["m"], "vcot": S * ns, "noise": S * (d["T"] - 1) * d["n_pert"]}


DESC_FIELDS = ("T", "zdim", "off_a", "off_dt", "N", "dt_fixed", "global_dim", "m", "state_cols", "n_pert", "fid_kind", "fid_form", "n_sub",
               "device", "wide")


class StandIn:
    """`_lib.lib` for the test: records the sweep's evaluation calls, hands out dummy handles, answers fixed strings, and lets every
    host-only function of the real library through."""

    def __init__(self, real):
        self.real, self.log, self.descs, self.fail = real, [], {}, {}      # fail: symbol -> the code it answers

    def __getattr__(self, name):
        if name in SYMBOL_ARGS:
            return lambda *args: self._evaluate(name, *args)
        if name.startswith("qc_sweep_") and name not in PASS_THROUGH:
            raise AttributeError(f"the stand-in does not know {name}")
        return getattr(self.real, name)

    def qc_sweep_create(self, d, out):
        d = d._obj
        fields = {f: getattr(d, f) for f in DESC_FIELDS}
        fields["reserved1"] = list(d.reserved1)
        fields["null"] = [f for f in ("G_drift", "G_drives", "G_pert", "goal_iso", "subspace") if not getattr(d, f)]
        self.log.append({"symbol": "qc_sweep_create", "desc": fields})
        if "qc_sweep_create" in self.fail:
            return self.fail["qc_sweep_create"]
        out._obj.value = 1000 + len(self.descs)
        self.descs[out._obj.value] = fields
        return 0

    def qc_sweep_destroy(self, h):
        self.log.append({"symbol": "qc_sweep_destroy"})

    def qc_sweep_kernel_name(self, h):
        return b"stand-in-sweep"

    def qc_sweep_last_error(self, h):
        return b"stand-in message of the NULL handle" if h is None else b"stand-in message of handle %d" % h.value

    def qc_fidelity_create_kind(self, kind, N, goal, device, out):
        if "qc_fidelity_create_kind" not in self.fail:
            out._obj.value = 7
        return self.fail.get("qc_fidelity_create_kind", 0)

    def qc_fidelity_eval(self, h, *args):
        return self.fail.get("qc_fidelity_eval", 0)

    def qc_fidelity_destroy(self, h):
        pass

    def qc_fidelity_last_error(self, h):
        return b"stand-in fidelity message of the NULL handle" if h is None else b"stand-in fidelity message of handle %d" % h.value

    def _evaluate(self, name, h, *args):
        names = SYMBOL_ARGS[name]
        assert len(args) == len(names), (name, len(args))
        given = dict(zip(names, args))
        entry = {"symbol": name, "S": int(given["S"]), "null": [n for n in names if n not in ("S", "stream") and not given[n]]}
        if name.endswith("_dev"):
            entry["stream"] = given["stream"]
        else:
            entry["inputs"] = {n: np.ctypeslib.as_array(given[n], shape=(cnt,)).tolist() if cnt else []
                               for n, cnt in input_lengths(self.descs[h.value], entry["S"]).items() if n in given and given[n]}
        self.log.append(entry)
        return self.fail.get(name, 0)


class _Stream:
    def __init__(self, cuda_stream):
        self.cuda_stream = cuda_stream


@pytest.fixture()
def standin(qc, monkeypatch):
    s = StandIn(qc._lib.lib)
    monkeypatch.setattr(qc._lib, "lib", s)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: _Stream(11))
    return s


# ---- handles and arguments --------------------------------------------------------------------------------------------------
X = np.array([[0, 1], [1, 0]], dtype=complex)
Y = np.array([[0, -1j], [1j, 0]], dtype=complex)
Zp = np.diag([1.0, -1.0]).astype(complex)


def make_handle(qc, which):
    if which == "two_drives":     # two drives, two perturbations, T = 4, two state columns, the timestep in the knot, a ket fidelity
        return qc.RolloutSweep(qc.QuantumSystem(Zp, [X, Y]), [Zp, X], 4, cols=2, goal=np.arange(8.0), fid_kind="ket")
    if which == "fixed_dt":       # one drive, no perturbations, dt_fixed, T = 2, no fidelity: n_deriv = m, empty theta, one interval
        return qc.RolloutSweep(qc.QuantumSystem(Zp, [X]), [], 2, cols=1, dt_fixed=0.1)
    if which == "one_pert":       # one drive, one perturbation, T = 3: the two-dimensional noise form
        return qc.RolloutSweep(qc.QuantumSystem(Zp, [X]), [Zp], 3, goal=np.arange(8.0), fid_kind="unitary")
    if which == "no_drives":      # refusals only: a handle without drives
        return qc.RolloutSweep(qc.QuantumSystem(Zp, []), [X], 3, cols=1)
    raise KeyError(which)


HANDLES = ("two_drives", "fixed_dt", "one_pert")
ENTRIES = ("eval", "grad", "param_grad", "vjp", "jvp", "hvp", "noise_eval", "noise_grad")
ENTRIES += tuple(e + "_device" for e in ENTRIES)
REQUIRED = {"Z", "init", "cot", "noise", "dZ", "dinit", "S", "dcot", "dnoise"}
_BASE = {n: 100.0 * (k + 1) for k, n in enumerate(("Z", "init", "theta", "scale", "weights", "cot", "vZ", "vinit", "vtheta", "vscale", "vcot",
                                                    "noise"))}


def host_shapes(sw):
    noise = (S, sw.T - 1) if sw.p == 1 else (S, sw.T - 1, sw.p)
    return {"Z": (sw.Z_len,), "init": (sw.ns,), "theta": (S, sw.p), "scale": (S, sw.m), "weights": (S,), "cot": (S, sw.ns), "vZ": (sw.Z_len,),
            "vinit": (sw.ns,), "vtheta": (S, sw.p), "vscale": (S, sw.m), "vcot": (S, sw.ns), "noise": noise}


def device_counts(sw):
    per_interval = S * (sw.T - 1)
    c = {"d" + n: int(np.prod(shape)) for n, shape in host_shapes(sw).items()}
    c.update(dfinals=S * sw.ns, dfids=S, dJ=1, dgrad=sw.Z_len, dgrad_samples=per_interval * sw.n_deriv, dgrad_init=S * sw.ns, dgrad_theta=S * sw.p,
             dgrad_scale=S * sw.m, dgrad_noise=per_interval * sw.p, dtfinals=S * sw.ns, dtfids=S, dtgrad=sw.Z_len,
             dtgrad_samples=per_interval * sw.n_deriv, dtgrad_init=S * sw.ns)
    return c


def argument(sw, name):
    """The value this test gives for the parameter `name` of any entry."""
    shapes = host_shapes(sw)
    if name in shapes:
        return _BASE[name] + np.arange(float(np.prod(shapes[name]))).reshape(shapes[name])
    if name == "S":
        return S
    if name == "stream":
        return _Stream(77)
    if name in ("dgrad_theta", "dvtheta", "dgrad_scale", "dvscale") and not (sw.p if name.endswith("theta") else sw.m):
        return None     # outputs and directions shaped like theta / scale are refused on a handle without perturbations / drives
    if name.startswith("d"):
        return torch.zeros(device_counts(sw)[name], dtype=torch.float64)
    return True     # finals, fids, per_sample, init_grad, params, with_controls


def describe(x):
    if isinstance(x, tuple):
        return [describe(v) for v in x]
    if isinstance(x, np.ndarray):
        return ["ndarray", list(x.shape), str(x.dtype)]
    return type(x).__name__


def outcome(standin, fn, *args, **kwargs):
    """One recorded call: what the library saw, and what came back or was raised."""
    standin.log = log = []
    try:
        result = fn(*args, **kwargs)
        standin.log = []        # what is destroyed once the result is dropped is not part of the call
        out = {"returns": describe(result)}
    except Exception as e:      # whatever is raised is part of the record
        standin.log = []
        out = {"raises": [type(e).__name__, str(e)]}
        if hasattr(e, "code"):
            out["code"] = e.code
    out["library"] = log
    return out


def entry_calls(standin, sw, entry):
    """{label: outcome}: every optional argument given, then each left out in turn: a switch (finals, per_sample, ...) turned off, anything
    else at its default, or None where it has none."""
    method = getattr(sw, entry)
    params = inspect.signature(method).parameters
    full = {n: argument(sw, n) for n in params}
    calls = {"all": outcome(standin, method, **full)}
    for n, p in params.items():
        if n not in REQUIRED:
            absent = False if isinstance(p.default, bool) else None if p.default is inspect.Parameter.empty else p.default
            calls["without " + n] = outcome(standin, method, **{**full, n: absent})
    return calls


def record_calls(qc, standin):
    rec = {}
    for which in HANDLES:
        rec[which + ".create"] = outcome(standin, make_handle, qc, which)
        sw = make_handle(qc, which)
        for entry in ENTRIES:
            for label, out in entry_calls(standin, sw, entry).items():
                rec[f"{which}.{entry}: {label}"] = out
        a = lambda n: argument(sw, n)
        # the sample count from the directions / the cotangents alone
        if sw.p:
            rec[which + ".jvp: S from vtheta"] = outcome(standin, sw.jvp, a("Z"), a("init"), None, None, None, vtheta=a("vtheta"))
            rec[which + ".eval: one-dimensional theta and scale"] = outcome(standin, sw.eval, a("Z"), a("init"), a("theta").ravel(), a("scale").ravel())
        rec[which + ".jvp: S from vscale"] = outcome(standin, sw.jvp, a("Z"), a("init"), None, None, None, vscale=a("vscale"))
        rec[which + ".hvp: S from cot"] = outcome(standin, sw.hvp, a("Z"), a("init"), a("cot"), None, vZ=a("vZ"))
        rec[which + ".eval_device: S from dfinals"] = outcome(standin, sw.eval_device, a("dZ"), a("dinit"), a("dtheta"), None, a("dfinals"), None)
        rec[which + ".scope"] = outcome(standin, lambda: tuple((getattr(sw, e + "_supported"), getattr(sw, e + "_unsupported_reason"))
                                                               for e in ("grad", "vjp", "jvp", "hvp", "noise")))
        rec[which + ".launch"] = outcome(standin, sw.launch, S)
        rec[which + ".kernel_name"] = outcome(standin, lambda: sw.kernel_name)
        rec[which + ".attributes"] = {k: v for k, v in vars(sw).items() if isinstance(v, (bool, int)) and not k.startswith("_")}
        rec[which + ".n_deriv"] = sw.n_deriv
        rec[which + ".close"] = outcome(standin, sw.close)
    return rec


def record_flags(qc, standin):
    """The flag table of `__init__`: every flag's bit in `wide`, `stored_states` in reserved1[0], the attributes, the refusals."""
    rec = {}
    sys1 = qc.QuantumSystem(Zp, [X])
    flags = ("wide_params", "wide_stored", "wide_tangent", "wide_noise", "wide_hessian", "wide64")
    for f in flags:
        rec[f"{f} without wide"] = outcome(standin, lambda: qc.RolloutSweep(None, [], 5, **{f: True, "stored_states": True}))
        kw = {"wide": True, f: True, "stored_states": f == "wide_stored"}
        rec[f"{f} with wide"] = outcome(standin, lambda: qc.RolloutSweep(sys1, [], 5, **kw))
        sw = qc.RolloutSweep(sys1, [], 5, **kw)
        rec[f"{f} attributes"] = {k: getattr(sw, k) for k in flags + ("wide", "stored_states")}
    rec["wide_stored without stored_states"] = outcome(standin, lambda: qc.RolloutSweep(None, [], 5, wide=True, wide_stored=True))
    rec["wide alone"] = outcome(standin, lambda: qc.RolloutSweep(sys1, [], 5, wide=True))
    rec["stored_states alone"] = outcome(standin, lambda: qc.RolloutSweep(sys1, [], 5, stored_states=True))
    rec["every flag"] = outcome(standin, lambda: qc.RolloutSweep(sys1, [], 5, wide=True, stored_states=True, **{f: True for f in flags}))
    rec["layout given"] = outcome(standin, lambda: qc.RolloutSweep(sys1, [Zp], 5, zdim=7, off_a=3, global_dim=2, subspace=[0, 1], fid_kind="unitary",
                                                                  goal=np.arange(8.0), fid_form=qc._lib.QC_FID_FORM_ABS2, device=3))
    return rec


def record_refusals(qc, standin):
    """One single-fault input for every ValueError of `RolloutSweep` and of the one-shot functions."""
    rec = {}
    handles = {w: make_handle(qc, w) for w in HANDLES + ("no_drives",)}

    def refuse(label, which, entry, **change):
        sw = handles[which]
        method = getattr(sw, entry)
        full = {n: argument(sw, n) for n in inspect.signature(method).parameters}
        rec[f"{which}.{entry}: {label}"] = outcome(standin, method, **{**full, **change})

    sw = handles["two_drives"]
    rec["generator shape"] = outcome(standin, lambda: qc.RolloutSweep(qc.QuantumSystem(Zp, [X]), [np.eye(3)], 3))
    rec["pack: controls"] = outcome(standin, sw.pack, np.zeros((2, 3)), 0.1)
    rec["pack: no timesteps"] = outcome(standin, sw.pack, np.zeros((2, 4)))
    rec["pack: accepted"] = outcome(standin, sw.pack, np.zeros((2, 4)), 0.1)
    rec["finals_autograd: no samples"] = outcome(standin, sw.finals_autograd, None, None)
    for label, change in (("neither theta nor scale", dict(theta=None, scale=None)), ("theta shape", dict(theta=np.zeros((S, 3)))),
                          ("theta required", dict(theta=None)), ("scale shape", dict(scale=np.zeros((S + 1, 2)))),
                          ("no sample", dict(theta=np.zeros((0, 2)), scale=None))):
        refuse(label, "two_drives", "eval", **change)
    for entry in ENTRIES[:8]:
        refuse("Z length", "two_drives", entry, Z=np.zeros(sw.Z_len + 1))
        refuse("init length", "two_drives", entry, init=np.zeros(sw.ns - 1))
    for entry in ("grad", "param_grad", "noise_grad"):
        refuse("weights", "two_drives", entry, weights=np.ones(S + 1))
    refuse("cot shape", "two_drives", "vjp", cot=np.zeros((S, sw.ns + 1)))
    refuse("cot size", "two_drives", "hvp", cot=np.zeros((S, sw.ns + 1)))
    for entry, names in (("jvp", ("vZ", "vinit", "vtheta", "vscale")), ("hvp", ("vZ", "vinit", "vtheta", "vscale", "vcot"))):
        for n in names:
            refuse(n + " size", "two_drives", entry, **{n: np.zeros(argument(sw, n).size + 1)})
    for entry in ("noise_eval", "noise_grad"):
        refuse("noise required", "two_drives", entry, noise=None)
        refuse("noise shape", "two_drives", entry, noise=np.zeros((S, 2, 2)))
        refuse("noise shape", "one_pert", entry, noise=np.zeros((S, 3)))
        refuse("samples of theta and noise", "two_drives", entry, theta=np.zeros((S + 1, 2)), scale=None)
    # device entries: every named tensor with one entry too many, one wrong type, one not contiguous; every refusal of its own
    for entry in ENTRIES[8:]:
        for n in inspect.signature(getattr(sw, entry)).parameters:
            if n.startswith("d") and not (n == "dnoise" or (entry == "eval_device" and n == "dfids")):
                refuse(n + " count", "two_drives", entry, **{n: torch.zeros(device_counts(sw)[n] + 1, dtype=torch.float64)})
        refuse("dZ type", "two_drives", entry, dZ=torch.zeros(sw.Z_len, dtype=torch.float32))
        refuse("dZ not contiguous", "two_drives", entry, dZ=torch.zeros(2 * sw.Z_len, dtype=torch.float64)[::2])
    for entry in ("eval_device", "noise_eval_device"):
        refuse("no output", "two_drives", entry, dfinals=None, dfids=None)
    refuse("no output", "two_drives", "grad_device", dfids=None, dJ=None, dgrad=None, dgrad_samples=None)
    refuse("no output", "two_drives", "param_grad_device", dfids=None, dJ=None, dgrad=None, dgrad_samples=None, dgrad_theta=None, dgrad_scale=None)
    refuse("no output", "two_drives", "vjp_device", dfinals=None, dgrad=None, dgrad_samples=None, dgrad_init=None, dgrad_theta=None, dgrad_scale=None)
    refuse("no output", "two_drives", "jvp_device", dfinals=None, dfids=None, dtfinals=None, dtfids=None)
    refuse("no output", "two_drives", "hvp_device", dtgrad=None, dtgrad_samples=None, dtgrad_init=None)
    refuse("no output", "two_drives", "noise_grad_device", dfids=None, dJ=None, dgrad=None, dgrad_samples=None, dgrad_noise=None)
    refuse("no direction", "two_drives", "jvp_device", dvZ=None, dvinit=None, dvtheta=None, dvscale=None)
    refuse("no direction", "two_drives", "hvp_device", dvZ=None, dvinit=None, dvtheta=None, dvscale=None, dvcot=None)
    for entry in ("vjp_device", "hvp_device"):
        refuse("dcot required", "two_drives", entry, dcot=None)
    for entry in ("grad_device", "param_grad_device", "vjp_device", "jvp_device", "hvp_device"):
        refuse("dtheta required", "two_drives", entry, dtheta=None)
    for entry, t, c in (("param_grad_device", "dgrad_theta", "dgrad_scale"), ("vjp_device", "dgrad_theta", "dgrad_scale"),
                        ("jvp_device", "dvtheta", "dvscale"), ("hvp_device", "dvtheta", "dvscale")):
        refuse(t + " without perturbations", "fixed_dt", entry, **{t: torch.zeros(0, dtype=torch.float64)})
        refuse(c + " without drives", "no_drives", entry, **{c: torch.zeros(0, dtype=torch.float64)})
    for entry in ("noise_eval_device", "noise_grad_device"):
        refuse("dnoise required", "two_drives", entry, dnoise=None)
        refuse("dnoise count", "two_drives", entry, dnoise=torch.zeros(S * 3 * 2 + 1, dtype=torch.float64))
        refuse("dnoise empty", "two_drives", entry, dnoise=torch.zeros(0, dtype=torch.float64))
        refuse("dnoise without perturbations", "fixed_dt", entry)
    for h in handles.values():
        h.close()
    return rec


def record_one_shots(qc, standin):
    """The three module-level functions: an accepted call each (flags included), and the refusal of their controls."""
    rec = {}
    sys2 = qc.QuantumSystem(Zp, [X, Y])
    init, controls = np.arange(8.0), 0.1 * np.arange(8.0).reshape(2, 4)
    theta, noise = 200.0 + np.arange(4.0).reshape(2, 2), 300.0 + np.arange(12.0).reshape(2, 3, 2)
    rec["rollout_sweep"] = outcome(standin, qc.rollout_sweep, init, controls, 0.1, sys2, [Zp, X], theta, goal=np.arange(8.0), fid_kind="unitary")
    rec["rollout_sweep: flags"] = outcome(standin, qc.rollout_sweep, init, controls, np.arange(4.0), sys2, [Zp, X], theta, np.ones((2, 2)), cols=2,
                                         subspace=[0], device=1, fid_form=1, wide=True, stored_states=True, wide_stored=True, wide_tangent=True,
                                         wide64=True)
    rec["rollout_noise_sweep"] = outcome(standin, qc.rollout_noise_sweep, init, controls, 0.1, sys2, [Zp, X], noise)
    rec["rollout_noise_sweep: flags"] = outcome(standin, qc.rollout_noise_sweep, init, controls, 0.1, sys2, [Zp, X], noise, theta, np.ones((2, 2)),
                                               cols=2, goal=np.arange(8.0), fid_kind="ket", device=1, fid_form=1, wide=True)
    rec["rollout_sweep_parameter_gradient"] = outcome(standin, qc.rollout_sweep_parameter_gradient, init, controls, 0.1, sys2, [Zp, X], theta,
                                                     goal=np.arange(8.0))
    rec["rollout_sweep_parameter_gradient: flags"] = outcome(standin, qc.rollout_sweep_parameter_gradient, init, controls, 0.1, sys2, [Zp, X], theta,
                                                            np.ones((2, 2)), goal=np.arange(8.0), fid_kind="ket", stored_states=True, wide=True,
                                                            wide_stored=True)
    for fn, extra in ((qc.rollout_sweep, (theta,)), (qc.rollout_noise_sweep, (noise,)), (qc.rollout_sweep_parameter_gradient, (theta,))):
        rec[fn.__name__ + ": controls"] = outcome(standin, fn, init, np.zeros((3, 4)), 0.1, sys2, [Zp, X], *extra)
        rec[fn.__name__ + ": controls not a matrix"] = outcome(standin, fn, init, np.zeros(4), 0.1, sys2, [Zp, X], *extra)
    return rec


def record_failures(qc, standin):
    """The library answers QC_ERR_HIP: the error carries the code, and the message of the handle -- of NULL where there is none."""
    rec = {}
    sw = make_handle(qc, "two_drives")
    standin.fail = {name: qc._lib.QC_ERR_HIP for name in list(SYMBOL_ARGS) + ["qc_sweep_create", "qc_fidelity_create_kind"]}
    for entry in ENTRIES:
        method = getattr(sw, entry)
        rec[entry] = outcome(standin, method, **{n: argument(sw, n) for n in inspect.signature(method).parameters})
    rec["create"] = outcome(standin, make_handle, qc, "fixed_dt")
    rec["fidelity create"] = outcome(standin, qc.iso_fidelity, np.arange(4.0), np.arange(4.0))
    standin.fail = {"qc_fidelity_eval": qc._lib.QC_ERR_INVALID}
    rec["fidelity eval"] = outcome(standin, qc.iso_fidelity, np.arange(4.0), np.arange(4.0))
    standin.fail = {}
    sw.close()
    return rec


def test_binding_calls_match_the_recorded_ones(qc, standin):
    rec = {"calls": record_calls(qc, standin), "flags": record_flags(qc, standin), "refusals": record_refusals(qc, standin),
           "one_shots": record_one_shots(qc, standin), "failures": record_failures(qc, standin)}
    rec = json.loads(json.dumps(rec))
    if RECORDING:
        with open(GOLDEN, "w") as f:
            f.write("{\n" + ",\n".join(f' {json.dumps(part)}: {{\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in calls.items())
                                       + "\n }" for part, calls in rec.items()) + "\n}\n")
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert list(rec) == list(golden)
    for part in rec:
        assert sorted(rec[part]) == sorted(golden[part]), part
        for label in rec[part]:
            assert rec[part][label] == golden[part][label], f"{part}: {label}"


def test_every_refusal_is_a_value_error_and_every_call_reaches_one_symbol(qc, standin):
    """The record's own shape: a refusal is a ValueError that reached no evaluation symbol; an accepted call reached exactly the symbol of
    its entry, once."""
    for label, out in record_refusals(qc, standin).items():
        if label != "pack: accepted":
            assert out.get("raises", [None])[0] == "ValueError" and not out["library"], (label, out)
    sw = make_handle(qc, "two_drives")
    for entry in ENTRIES:
        out = entry_calls(standin, sw, entry)["all"]
        symbol = "qc_sweep_" + entry.replace("param_grad", "grad_params").replace("_device", "_dev")
        assert "returns" in out and [c["symbol"] for c in out["library"]] == [symbol], (entry, out)
    sw.close()
