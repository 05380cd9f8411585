"""No GPU: the momentum march -- a vector field that advects itself -- on the CPU.  The momentum functions of tests/march_ref.py
(the stage restated from its step in a velocity) against what they are built from, the oblique steady viscous shock, and the
argument checks of ``momentum_step`` / ``momentum_march`` (pyapes_amd/solver/march.py), which fire before a device is touched.

Oblique steady viscous shock (measured on the CPU, printed by the test): with the unit vector n = (1, 1) / sqrt(2) and
s = n . (x - x0), U = -A n tanh(A s / (2 nu)) is a steady solution of the advective-form momentum equation (u u' = nu u'').
A = 1, nu = 0.05 on [0, 1]^2, x0 the centre, dirichlet faces holding the exact values as per-component face arrays, started
from the exact field and marched with order 3 to T = 0.2 at dt = 0.4 dx^2 / (4 nu).  Max-abs error against the exact field at
33^2 / 65^2:
    upwind  0.03126 / 0.01712    (ratio 1.83, observed order 0.87)
    QUICK   0.002104 / 0.0005407 (ratio 3.89, observed order 1.96)
QUICK / upwind: 0.067 at 33^2, 0.032 at 65^2.  The two components differ by exactly 0: with n on the diagonal they are the same
function with the same face values, and each is stepped by the same operations on the same operands.  Asserted: both errors
fall under refinement, QUICK's is below upwind's at both resolutions, and the components agree to a few units of rounding --
no figure nobody has derived.  (Central Div is the conservative form div(u phi): for a field with divergence it solves
another equation, so it is not part of this check.)
"""
import math

import pytest
import torch

import march_ref as R
import pyapes_oracle as O
from march_ref import momentum as MR
from pyapes_amd.solver import march as M
from pyapes_amd.solver.march import euler_march, euler_step, momentum_march, momentum_step, rk_march, rk_step


# ---- the restatement ------------------------------------------------------------------------------------------------
def _vector_case(n, dtype, seed=11):
    """oracle mesh, one oracle BC list per component (same types, other values), a BC-filled vector field, sources"""
    nd = len(n)
    mesh = O.OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
    tdt = torch.float64 if dtype == "double" else torch.float32
    g = torch.Generator().manual_seed(seed)
    types = ["dirichlet", "neumann", "symmetry", "dirichlet", "neumann", "dirichlet"][:2 * nd]
    bcs = []
    for c in range(nd):
        vals = [0.5 - c, 0.1 * (c + 1), None, 1.0 + 0.25 * c, -0.3 * (c + 1), 0.125 * c][:2 * nd]
        bcs.append(O.make_bcs(mesh, O.mixed_cfg(vals, types, O.FACES[:2 * nd])))
    U = torch.randn((nd, *n), generator=g, dtype=torch.float64).to(tdt)
    for c in range(nd):
        O.bc_fill(U[c:c + 1], bcs[c])
    S = [torch.randn(tuple(n), generator=g, dtype=torch.float64).to(tdt) for _ in range(nd)]
    return mesh, bcs, U, S


@pytest.mark.parametrize("limiter", ["upwind", "quick"])
@pytest.mark.parametrize("n,dtype", [([7, 9, 12], "single"), ([17, 12], "double")], ids=["3d_f32", "2d_f64"])
def test_a_stage_is_the_velocity_step_of_every_component(n, dtype, limiter):
    """component c of a stage is march_ref's step of V_c in the velocity V with c's BCs, computed from the INPUT: stepping
    the components one after another in place (each seeing its predecessors' output) is another result"""
    mesh, bcs, U, S = _vector_case(n, dtype)
    nd = len(n)
    nu, dt = 0.05, 1e-3
    got = MR.euler_step(U, nu, dt, mesh, bcs, limiter, S)
    vel = [U[a] for a in range(nd)]
    for c in range(nd):
        assert torch.equal(got[c:c + 1], R.euler_step(U[c:c + 1], vel, nu, dt, mesh, bcs[c], limiter, S[c]))
    seq = U.clone()
    for c in range(nd):
        seq[c:c + 1] = R.euler_step(seq[c:c + 1], [seq[a] for a in range(nd)], nu, dt, mesh, bcs[c], limiter, S[c])
    assert not torch.equal(seq, got)
    # the frozen form is d scalar marches; every stage of the self form is advected by its own input
    frozen = [U[a].clone() for a in range(nd)]
    m = MR.march(U, nu, dt, 2, mesh, bcs, limiter, 3, S, u=frozen)
    for c in range(nd):
        assert torch.equal(m[c:c + 1], R.march(U[c:c + 1], frozen, nu, dt, 2, mesh, bcs[c], limiter, 3, S[c]))
    assert not torch.equal(MR.march(U, nu, dt, 2, mesh, bcs, limiter, 3, S), m)
    one = MR.march(U, nu, dt, 1, mesh, bcs, limiter, 2)
    e = MR.euler_step(U, nu, dt, mesh, bcs, limiter)
    assert torch.equal(one, MR.rk_stage(e, U, 0.5, 0.5, nu, dt, mesh, bcs, limiter))


def _shock_error(N, limiter, T=0.2, A=1.0, nu=0.05):
    mesh = O.OMesh([0.0, 0.0], [1.0, 1.0], [N, N], "double")
    x, y = mesh.grid
    s = ((x - 0.5) + (y - 0.5)) / math.sqrt(2.0)
    comp = -A / math.sqrt(2.0) * torch.tanh(A * s / (2.0 * nu))
    exact = torch.stack([comp, comp])
    bcs = [O.make_bcs(mesh, [{"bc_face": f, "bc_type": "dirichlet", "bc_val": exact[c][mesh.face_mask(f)].clone()}
                             for f in O.FACES[:4]]) for c in range(2)]
    dx = 1.0 / (N - 1)
    nsteps = int(math.ceil(T / (0.4 * dx * dx / (4.0 * nu))))
    end = MR.march(exact.clone(), nu, T / nsteps, nsteps, mesh, bcs, limiter, 3)
    return float((end - exact).abs().max()), float((end[0] - end[1]).abs().max())


def test_oblique_steady_viscous_shock():
    res = {lim: [_shock_error(N, lim) for N in (33, 65)] for lim in ("quick", "upwind")}
    err = {lim: [r[0] for r in v] for lim, v in res.items()}
    for lim, (e1, e2) in err.items():
        print(f"shock {lim}: max error 33^2 {e1:.4g}, 65^2 {e2:.4g}, ratio {e1 / e2:.3f}, observed order {math.log2(e1 / e2):.2f}")
    print(f"shock quick / upwind: 33^2 {err['quick'][0] / err['upwind'][0]:.3f}, 65^2 {err['quick'][1] / err['upwind'][1]:.3f}")
    print("shock component difference:", {lim: [r[1] for r in v] for lim, v in res.items()})
    for lim in err:
        assert err[lim][1] < err[lim][0], err
    for q, p in zip(err["quick"], err["upwind"]):
        assert q < p, err
    # |U| <= 1 / sqrt(2): 16 units of double rounding at that size
    for v in res.values():
        for _, d in v:
            assert d <= 16 * 2.0 ** -53, res


# ---- the checks in front of the device ------------------------------------------------------------------------------
def _cpu_field(n=(9, 9), dim=None, slab=None, geo=None, dtype="double"):
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    box = geo if geo is not None else (Box[0:1] if len(n) == 1 else (Box[0:1, 0:1] if len(n) == 2 else Box[0:1, 0:1, 0:1]))
    kw = {"slab": slab} if slab else {}
    mesh = Mesh(box, None, list(n), "cpu", dtype, **kw)
    cfg = mixed_bcs([0.0] * (2 * len(n)), ["dirichlet"] * (2 * len(n)))
    if geo is not None:
        cfg = [dict(c, bc_face=f) for c, f in zip(cfg, O.FACES_RZ)]
    return Field("U", len(n) if dim is None else dim, mesh, {"domain": cfg, "obstacle": None})


def _same_mesh_field(U):
    from pyapes_amd.variables.bcs import mixed_bcs
    return type(U)("S", 2, U.mesh, {"domain": mixed_bcs([0.0] * 4, ["dirichlet"] * 4), "obstacle": None})


def _calls(U, **kw):
    order = kw.pop("order", None)
    orders = (1, 2, 3) if order is None else (order,)
    out = []
    for o in orders:
        out.append(lambda o=o: momentum_step(U, 0.05, 1e-3, order=o, **kw))
        out.append(lambda o=o: momentum_march(U, 0.05, 1e-3, 2, order=o, **kw))
    return out


@pytest.fixture
def no_device(monkeypatch):
    """a refusal must come before context_for (and before require_gpu) is reached"""
    def reached(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(M, "context_for", reached)
    monkeypatch.setattr(M, "require_gpu", reached)


def test_momentum_argument_checks_fire_before_a_device_is_touched(no_device):
    from pyapes_amd.geometry import Cylinder
    U = _cpu_field()
    comp = U()[0].shape
    good = torch.zeros(comp, dtype=torch.float64)
    not_implemented = [
        (_cpu_field(dim=1), {}),                                               # U.dim != mesh.dim
        (_cpu_field(dim=3), {}),
        (_cpu_field(n=(9,)), {}),                                              # a 1-D mesh: rk_march(phi, phi)
        (_cpu_field(n=(9, 9, 9), slab=(0, 2)), {}),
        (_cpu_field(geo=Cylinder[0:1, 0:1]), {}),
        (U, {"config": {"div": {"limiter": "upwind", "compat": True}}}),
        (U, {"u": U}),                                                         # u= on U's storage: that is u=None
        (U, {"u": U()}),
        (U, {"u": (U()[0], 1.0)}),
        (U, {"u": (good, U()[1])}),
    ]
    for f, kw in not_implemented:
        for call in _calls(f, **kw):
            with pytest.raises(NotImplementedError):
                call()
    other = _cpu_field()
    src_field = _cpu_field()
    src_field.set_var_tensor(torch.ones_like(U()))
    value_errors = [
        {"order": 4}, {"order": 0},
        {"source": [1.0]}, {"source": (1.0, 2.0, 3.0)},                       # wrong number of entries
        {"source": [good, torch.zeros(9, 8, dtype=torch.float64)]},           # wrong shape
        {"source": torch.zeros(3, 9, 9, dtype=torch.float64)},
        {"source": torch.zeros(9, 9, dtype=torch.float64)},
        {"source": [good, torch.zeros(comp, dtype=torch.float32)]},           # wrong dtype
        {"source": [good, torch.zeros(comp, dtype=torch.float64, device="meta")]},   # wrong device
        {"source": [U()[0], 1.0]},                                             # on U's storage
        {"source": U()},
        {"source": other},                                                     # a Field on another mesh
        {"source": _cpu_field(dim=1)},
        {"u": (1.0,)}, {"u": [1.0, 2.0, 3.0]},                                 # the velocity's own checks
        {"u": (good, torch.zeros(9, 8, dtype=torch.float64))},
        {"u": (good, torch.zeros(comp, dtype=torch.float32))},
        {"u": other},
    ]
    for kw in value_errors:
        for call in _calls(U, **dict(kw)):
            with pytest.raises(ValueError):
                call()
    type_errors = [{"source": [good, "big"]}, {"source": [True, 1.0]}, {"source": 1.0}, {"source": "S"},
                   {"u": (good, "fast")}, {"u": (True, 1.0)}, {"u": 1.0}, {"u": torch.ones(1, 9, 9, dtype=torch.float64)}]
    for kw in type_errors:
        for call in _calls(U, **dict(kw)):
            with pytest.raises(TypeError):
                call()
    # a source Field of the same mesh is the one good Field
    assert M._momentum_args(U, None, 3, None, _same_mesh_field(U), "momentum_step")[2] is not None


def test_good_arguments_reach_the_context(monkeypatch):
    """every accepted form of ``u=`` and ``source=`` arrives at Context.momentum_march as the lists the checks make of it"""
    U = _cpu_field()
    U.set_var_tensor(torch.arange(162, dtype=torch.float64).reshape(2, 9, 9))
    U.set_time(0.0, 1.5)
    comp = U()[0].shape
    t = torch.arange(81, dtype=torch.float64).reshape(comp)
    t2 = -t.clone()
    vecf = _same_mesh_field(U)
    vecf.set_var_tensor(torch.stack([t, t2]))
    seen = []

    class Recorder:
        def bind_bcs(self, var, bcs, comp_=0, **k):
            seen.append(("bind", comp_))

        def momentum_march(self, U_, w1, w2, order, kind, vel, nu, dt, nsteps, sources, bcs):
            assert U_.is_contiguous() and U_.shape == w1.shape and (w2 is None) == (order == 1) and bcs is U.bcs
            seen.append((order, vel, sources, nsteps))
            return w1

        def __getattr__(self, name):
            raise AssertionError(f"the momentum march went to Context.{name}")

    monkeypatch.setattr(M, "context_for", lambda mesh: Recorder())
    monkeypatch.setattr(M, "require_gpu", lambda *a, **k: None)

    def same(got, want):
        if want is None:
            assert got is None
            return
        assert len(got) == len(want)
        for g, w in zip(got, want):
            if isinstance(w, torch.Tensor):
                assert isinstance(g, torch.Tensor) and g.is_contiguous() and torch.equal(g, w)
            elif w is None:
                assert g is None
            else:
                assert isinstance(g, float) and g == w

    vels = [(None, None), ((1.0, -2.0), [1.0, -2.0]), ([1, 0.5], [1.0, 0.5]), ((t, 2.0), [t, torch.full_like(t, 2.0)]),
            ((t, t2), [t, t2]), (torch.stack([t, t2]), [t, t2]), (vecf, [t, t2])]
    sources = [(None, None), ([1.5, None], [1.5, None]), ((t, -2), [t, -2.0]), ([t.unsqueeze(0), t2], [t, t2]),
               (torch.stack([t, t2]), [t, t2]), (vecf, [t, t2])]
    for u, want_u in vels:
        for s, want_s in sources:
            del seen[:]
            calls = _calls(U, u=u, source=s)
            t_before = float(U.t)
            for call in calls:
                assert call() is U
            marches = [e for e in seen if e[0] != "bind"]
            assert len(marches) == len(calls) and sum(1 for e in seen if e == ("bind", 0)) == len(calls)
            for (order, vel, srcs, nsteps), o in zip(marches, (1, 1, 2, 2, 3, 3)):
                assert order == o
                same(vel, want_u)
                same(srcs, want_s)
            assert [e[3] for e in marches] == [1, 2] * 3
            # momentum_march advances the time by nsteps * dt, momentum_step does not
            assert abs(float(U.t) - (t_before + 3 * 2 * 1e-3)) <= 1e-12
    # the limiter reaches the Context as the Div kind
    from pyapes_amd.solver.fdc import div_kind
    for lim in ("upwind", "quick", "none"):
        kinds = []
        monkeypatch.setattr(Recorder, "momentum_march", lambda self, U_, w1, w2, order, kind, *a: kinds.append(kind) or w1)
        momentum_step(U, 0.05, 1e-3, {"div": {"limiter": lim}})
        assert kinds == [div_kind(lim, False)]


def test_the_scalar_entry_points_still_refuse_vector_targets():
    vec = _cpu_field()
    for u in (vec, (1.0, 2.0)):
        for call in (lambda: euler_march(vec, u, 0.05, 1e-3, 2), lambda: rk_step(vec, u, 0.05, 1e-3),
                     lambda: rk_march(vec, u, 0.05, 1e-3, 2)):
            with pytest.raises(NotImplementedError):
                call()
    with pytest.raises(NotImplementedError):
        euler_step(vec, (1.0, 2.0), 0.05, 1e-3)
