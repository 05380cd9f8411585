"""Context reuse: replay a script of operations on ONE mesh (one ``pa_ctx``) and compare every step with the same operation
on a mesh that has seen nothing else.  A plain module, no test lives here: tests/test_ctx_reuse_host.py checks the runners
on fake operations (no GPU), tests/test_gpu_ctx_reuse.py holds the scripts.

The runners
    An operation is ``op(mesh, carried) -> dict`` of CPU tensors and reports (``Op`` below).  Its inputs are seeded, or taken
    from ``carried.fields`` (CPU tensors a script hands from step to step); options it sets go into ``carried.options``.
    ``run_script(ops, make_mesh)`` runs all of them on one mesh, ``run_fresh(op, before, make_mesh)`` one of them on a newly
    built mesh with the carried state ``before`` copied in and the options of ``before`` set on its new context.
    ``verify`` asserts that EVERY step of the script equals its fresh run: ``torch.equal`` on tensors, ``==`` on everything
    else (a NaN equals a NaN), the same keys on both sides, and as many compared steps as the script has.

Poisoning
    After each step ``run_script`` fills with NaN every device tensor the caller owns that an earlier step (that one
    included) handed to the library -- what the operations register with ``carried.own`` -- and every tensor the context's
    Python side held for the library after an earlier step and has dropped since.  A kernel that still reads a pointer of
    an earlier binding then produces NaN, not a near miss.

The catalogue (GPU) is below the runners; it goes through the public Python layer only.
"""
from __future__ import annotations

import math
import warnings
from typing import Any, Callable, Sequence

import torch
from torch import Tensor


# ======================================================================================================================
#  the runners (no GPU needed: tests/test_ctx_reuse_host.py)
# ======================================================================================================================
class Carried:
    """What a script carries from step to step: CPU tensors, the options set on the context so far, and the tensors the
    caller owns that the library was handed (``own``)."""

    def __init__(self, fields: dict[str, Tensor] | None = None, options: dict[str, int] | None = None):
        self.fields = dict(fields or {})
        self.options = dict(options or {})
        self.owned: list[Tensor] = []

    def own(self, *tensors: Tensor | None) -> None:
        self.owned += [t for t in tensors if isinstance(t, Tensor)]

    def snapshot(self) -> "Carried":
        return Carried({k: v.clone() for k, v in self.fields.items()}, self.options)


class Op:
    """``fn(mesh, carried) -> dict``.  ``key`` names the distinct operation (the independent reference runs once per key);
    ``pure``: the result depends on nothing carried, so every occurrence in a script must give the same result;
    ``ref(before, out, geometry)``: asserts ``out`` against an independent CPU reference; ``geometry`` is whatever the
    script's caller hands ``check_script`` for that purpose (the GPU scripts: the same mesh built on the CPU)."""

    def __init__(self, name: str, fn: Callable[[Any, Carried], dict], ref: Callable[[Carried, dict, Any], None] | None = None,
                 pure: bool = False, key: str | None = None):
        self.name, self.fn, self.ref, self.pure, self.key = name, fn, ref, pure, key or name

    def __call__(self, mesh: Any, carried: Carried) -> dict:
        return self.fn(mesh, carried)


class Step:
    def __init__(self, k: int, op: Op, before: Carried, out: dict):
        self.k, self.op, self.before, self.out = k, op, before, out


def _tensors_in(obj: Any, found: dict[int, Tensor]) -> None:
    if isinstance(obj, Tensor):
        found[id(obj)] = obj
    elif isinstance(obj, dict):
        for v in obj.values():
            _tensors_in(v, found)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors_in(v, found)


def held_by_context(mesh: Any) -> dict[int, Tensor]:
    """the tensors the Python side of ``mesh``'s context keeps alive because the library holds their pointers"""
    found: dict[int, Tensor] = {}
    ctx = getattr(mesh, "_hip", None)
    _tensors_in(getattr(ctx, "_keep", None), found)
    return found


def poison(tensors: Sequence[Tensor]) -> None:
    for t in tensors:
        if t.is_floating_point():
            t.fill_(float("nan"))


def _sync() -> None:
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def set_options(mesh: Any, options: dict[str, int]) -> None:
    from pyapes_amd.hip.context import context_for
    for name, value in options.items():
        context_for(mesh).set_option(name, value)


def run_script(ops: Sequence[Op], make_mesh: Callable[[], Any], poisoning: bool = True) -> list[Step]:
    """all ops in order on ONE mesh; the inputs of the steps behind are poisoned after every step"""
    mesh = make_mesh()
    carried = Carried()
    dropped: dict[int, Tensor] = {}     # once held for the library by the context
    steps = []
    for k, op in enumerate(ops):
        before = carried.snapshot()
        out = op(mesh, carried)
        _sync()
        steps.append(Step(k, op, before, out))
        held = held_by_context(mesh)
        if poisoning:
            poison(carried.owned)
            poison([t for i, t in dropped.items() if i not in held])
            _sync()
        dropped.update(held)
    return steps


def run_fresh(op: Op, before: Carried, make_mesh: Callable[[], Any], configure: Callable[[Any, dict], None] = set_options) -> dict:
    """one op on a newly built mesh of the same geometry, the carried state copied in"""
    mesh = make_mesh()
    carried = before.snapshot()
    configure(mesh, carried.options)
    out = op(mesh, carried)
    _sync()
    return out


def differences(a: Any, b: Any, where: str = "") -> list[str]:
    """what differs between two results, exactly: no tolerance anywhere"""
    if isinstance(a, dict) or isinstance(b, dict):
        if not (isinstance(a, dict) and isinstance(b, dict)) or set(a) != set(b):
            return [f"{where}: keys {sorted(a) if isinstance(a, dict) else a} != {sorted(b) if isinstance(b, dict) else b}"]
        return [d for key in sorted(a) for d in differences(a[key], b[key], f"{where}.{key}" if where else str(key))]
    if isinstance(a, Tensor) or isinstance(b, Tensor):
        if not (isinstance(a, Tensor) and isinstance(b, Tensor)) or a.shape != b.shape or a.dtype != b.dtype:
            return [f"{where}: tensors of different kinds"]
        if torch.equal(a, b):
            return []
        both_nan = torch.isnan(a) & torch.isnan(b) if a.is_floating_point() else torch.zeros_like(a, dtype=torch.bool)
        bad = (a != b) & ~both_nan
        if not bool(bad.any()):
            return []
        nan = int(torch.isnan(a).sum()) if a.is_floating_point() else 0
        nan_b = int(torch.isnan(b).sum()) if b.is_floating_point() else 0
        return [f"{where}: {int(bad.sum())} of {a.numel()} entries differ ({nan} NaN here, {nan_b} in the fresh run)"]
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return []
    return [] if (type(a) is type(b) and a == b) else [f"{where}: {a!r} != {b!r}"]


def verify(steps: Sequence[Step], fresh: dict[int, dict], n_script: int) -> None:
    """every step of the script equals its fresh run -- and every step WAS compared"""
    problems, compared = [], 0
    for s in steps:
        if s.k not in fresh:
            continue
        compared += 1
        d = differences(s.out, fresh[s.k])
        if d:
            problems.append(f"step {s.k} ({s.op.name}) differs from its fresh run: " + "; ".join(d))
    assert compared == n_script == len(steps), f"{compared} steps compared, the script has {n_script} ({len(steps)} ran)"
    first: dict[str, Step] = {}
    for s in steps:       # an operation that depends on nothing carried gives the same result wherever it stands
        if s.op.pure and s.before.options == first.setdefault(s.op.key, s).before.options:
            d = differences(s.out, first[s.op.key].out)
            if d:
                problems.append(f"step {s.k} ({s.op.name}) differs from its first occurrence, step {first[s.op.key].k}: " + "; ".join(d))
    assert not problems, "\n".join(problems)


def check_script(ops: Sequence[Op], make_mesh: Callable[[], Any], configure: Callable[[Any, dict], None] = set_options,
                 poisoning: bool = True, geometry: Any = None) -> list[Step]:
    """run the script, every step fresh, the independent reference once per distinct operation; returns the script's steps"""
    steps = run_script(ops, make_mesh, poisoning)
    fresh, checked = {}, set()
    for s in steps:
        fresh[s.k] = run_fresh(s.op, s.before, make_mesh, configure)
        seen = (s.op.key, tuple(sorted(s.before.options.items())))
        if s.op.ref is not None and seen not in checked:
            s.op.ref(s.before, fresh[s.k], geometry)
            if s.op.pure:      # (an operation on carried fields is a distinct operation at every step)
                checked.add(seen)
    verify(steps, fresh, len(ops))
    return steps


# ======================================================================================================================
#  the catalogue: operations through the public Python layer (GPU)
# ======================================================================================================================
D = lambda v=0.0: ("dirichlet", v)   # noqa: E731
N = lambda v=0.0: ("neumann", v)     # noqa: E731
SY = ("symmetry", None)
PE = ("periodic", None)
NODES = "nodes"     # a Dirichlet face with one value per node: a face-value ARRAY the caller owns
BCSETS = {
    "dir": [D(0.0), D(0.5), D(0.0), D(0.0), D(1.0), D(0.0)],
    "mix": [N(0.3), D(0.0), D(0.3), N(0.0), SY, N(-0.25)],
    "mixv": [N(0.3), D(NODES), D(0.3), N(0.0), SY, N(-0.25)],
    "per": [PE] * 6,
    "xper": [PE, PE, D(0.0), D(1.0), N(0.0), SY],
    "dn": [D(0.4), N(0.25), SY, D(-0.3), N(0.0), D(1.0)],
}
UPPER = [1.0, 1.1, 0.5]


class MeshFactory:
    """``factory()``: a new mesh on the GPU; ``factory.cpu()``: the same geometry on the CPU, what the references restate"""

    def __init__(self, n: Sequence[int], dtype: str, rz: bool = False):
        self.n, self.dtype, self.rz = list(n), dtype, rz

    def _make(self, device: str) -> Any:
        from pyapes_amd.geometry import Box, Cylinder
        from pyapes_amd.mesh import Mesh
        geo = Cylinder([0.0, 0.0], [1.0, 1.5]) if self.rz else Box([0.0] * len(self.n), UPPER[:len(self.n)])
        return Mesh(geo, None, list(self.n), device, self.dtype)

    def __call__(self) -> Any:
        return self._make("cuda")

    def cpu(self) -> Any:
        return self._make("cpu")


def box_mesh(n: Sequence[int], dtype: str) -> MeshFactory:
    return MeshFactory(n, dtype)


def rz_mesh(n: Sequence[int], dtype: str) -> MeshFactory:
    return MeshFactory(n, dtype, rz=True)


def _omesh(mesh: Any):
    import pyapes_oracle as O
    nd = mesh.dim
    if mesh.coord_sys == "rz":
        return O.OMesh([0.0, 0.0], [1.0, 1.5], [int(v) for v in mesh.nx], _dtype_name(mesh), "rz")
    return O.OMesh([0.0] * nd, UPPER[:nd], [int(v) for v in mesh.nx], _dtype_name(mesh))


def _dtype_name(mesh: Any) -> str:
    return "double" if mesh.dtype.float == torch.float64 else "single"


def _faces(mesh: Any) -> list[str]:
    import pyapes_oracle as O
    return O.FACES_RZ if mesh.coord_sys == "rz" else O.FACES[:2 * mesh.dim]


def bc_configs(mesh: Any, faces: Sequence[tuple], order: Sequence[int] | None, seed: int):
    """(config of the Field with device face arrays, config of the oracle with their CPU copies, the device arrays)"""
    names = _faces(mesh)
    faces = list(faces)[:len(names)]
    g = torch.Generator().manual_seed(1000 + seed)
    dev_cfg, cpu_cfg, arrays = [], [], []
    for i, (t, v) in enumerate(faces):
        vd = vc = v
        if v == NODES:
            count = 1
            for a in range(mesh.dim):
                if a != i // 2:
                    count *= int(mesh.nx[a])
            vc = torch.randn(count, generator=g, dtype=torch.float64).to(mesh.dtype.float)
            vd = vc.to(mesh.device)
            arrays.append(vd)
        dev_cfg.append({"bc_face": names[i], "bc_type": t, "bc_val": vd, "bc_val_opt": None})
        cpu_cfg.append({"bc_face": names[i], "bc_type": t, "bc_val": vc})
    if order is not None:
        dev_cfg, cpu_cfg = [dev_cfg[i] for i in order], [cpu_cfg[i] for i in order]
    return dev_cfg, cpu_cfg, arrays


def _rand(mesh: Any, seed: int, lead: int = 1, scale: float = 1.0) -> Tensor:
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn((lead, *[int(v) for v in mesh.nx]), generator=g, dtype=torch.float64)).to(mesh.dtype.float)


def _bars(mesh: Any) -> float:
    """the suite's bar of a solver iterate against the oracle"""
    return 1e-10 if mesh.dtype.float == torch.float64 else 1e-5


def _rel(a: Tensor, b: Tensor) -> float:
    a, b = a.double(), b.double()
    return float(torch.linalg.norm(a - b)) / max(float(torch.linalg.norm(b)), 1e-300)


def _report(mesh: Any, rep: Any) -> dict:
    from pyapes_amd.hip.context import context_for
    ctx = context_for(mesh)
    itr, tol = (rep["itr"], rep["tol"]) if isinstance(rep, dict) else (rep.itr, rep.tol)
    return {"itr": int(itr), "tol": float(tol), "scalars": ctx.scalars(), "resident_used": ctx.resident_used()}


def _quiet(fn: Callable[[], Any]) -> Any:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn()


def solve_op(method: str, bcname: str, sweeps: int, *, eq: str = "lap", seed: int = 7, order: Sequence[int] | None = None,
             save_old: bool = False, carried_x: str | None = None, carried_rhs: str | None = None, name: str | None = None,
             want_resident: bool | None = None) -> Op:
    """``Solver.set_eq`` + ``solve`` of a new Field: ``sweeps`` iterations (tol -1).  eq: "lap" -0.7 lap(p), "gamma"
    -lap(Gamma, p) with a tensor Gamma, "advdiff" div(u, p) - 0.05 lap(p) with upwind and a tensor u (BiCGSTAB).
    carried_x / carried_rhs: the start / the right-hand side come from the carried fields (and the result goes back)."""
    max_it = sweeps if method == "bicgstab" else sweeps - 1
    faces = BCSETS[bcname]
    name = name or f"{method}{sweeps}-{bcname}-{eq}" + ("" if order is None else "-shuffled") + ("-old" if save_old else "")

    def inputs(mesh: Any, carried: Carried):
        rhs = carried.fields[carried_rhs].clone() if carried_rhs else _rand(mesh, seed)
        if all(t == "periodic" for t, _ in faces[:2 * mesh.dim]):
            rhs -= rhs.mean()
        x0 = carried.fields[carried_x].clone() if carried_x else None
        gamma = (1.0 + 0.2 * torch.rand(rhs.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)).to(rhs.dtype)
        u = _rand(mesh, seed + 2, scale=0.6)
        return rhs, x0, gamma, u

    def fn(mesh: Any, carried: Carried) -> dict:
        from pyapes_amd.solver.fdm import FDM
        from pyapes_amd.solver.ops import Solver
        from pyapes_amd.variables import Field
        rhs, x0, gamma, u = inputs(mesh, carried)
        cfg, _, arrays = bc_configs(mesh, faces, order, seed)
        var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
        if x0 is not None:
            var.set_var_tensor(x0.cuda())
        rhs_d, gamma_d, u_d = rhs.cuda(), gamma.cuda(), u.cuda()
        c = {"method": method, "tol": -1.0, "max_it": max_it, "report": False}
        if save_old:
            c["save_old"] = True
        s = Solver({"fdm": c})
        if eq == "lap":
            s.set_eq(-FDM().laplacian(0.7, var) == rhs_d)
        elif eq == "gamma":
            s.set_eq(-FDM().laplacian(gamma_d, var) == rhs_d)
        else:
            fdm = FDM({"div": {"limiter": "upwind", "edge": False, "compat": True}})   # (the form the oracle has tables for)
            s.set_eq(fdm.div(u_d, var) - fdm.laplacian(0.05, var) == rhs_d)
        rep = _quiet(s.solve)
        out = {"x": var().cpu(), "rhs": rhs_d.cpu(), **_report(mesh, rep)}
        if save_old:
            out["x_old"] = var.VARo.cpu()
            carried.own(var.VARo)
        if carried_x:
            carried.fields[carried_x] = out["x"].clone()
        carried.own(var(), rhs_d, gamma_d, u_d, *arrays)
        if want_resident is not None:
            assert (out["resident_used"] > 0) == want_resident, (name, out["resident_used"])
        return out

    def ref(before: Carried, out: dict, mesh: Any) -> None:
        import pyapes_oracle as O
        om = _omesh(mesh)
        rhs, x0, gamma, u = inputs(mesh, before)
        _, ocfg, _ = bc_configs(mesh, faces, order, seed)
        if eq == "advdiff":     # (the oracle's loop on the right-hand side as set_eq adjusted it: tests/test_gpu_tiled_advdiff.py)
            obcs = O.make_bcs(om, ocfg)
            x = torch.zeros_like(rhs) if x0 is None else x0
            terms = [O.OTerm("div", O.div_tables(u, x, om, obcs, "upwind"), None, 1.0),
                     O.OTerm("laplacian", O.laplacian_tables(x, om, obcs), 0.05, -1.0)]
            fn_o = {"cg": O.cg, "bicgstab": O.bicgstab, "jacobi": O.jacobi}[method]
            xo, ro = _quiet(lambda: fn_o(x.clone(), out["rhs"].clone(), terms, om, obcs, -1.0, max_it))
        else:
            coeff = 0.7 if eq == "lap" else gamma
            xo, ro = _quiet(lambda: O.solve_poisson(om, ocfg, rhs.clone(), x0=x0, method=method, tol=-1.0, max_it=max_it,
                                                    coeff=coeff, sign=-1.0))
        assert out["itr"] == ro["itr"] == sweeps, (name, out["itr"], ro["itr"])
        assert _rel(out["x"], xo) < _bars(mesh), (name, _rel(out["x"], xo))

    return Op(name, fn, ref, pure=carried_x is None and carried_rhs is None)


def check_gpu_script(ops: Sequence[Op], make_mesh: MeshFactory, poisoning: bool = True) -> list[Step]:
    return check_script(ops, make_mesh, poisoning=poisoning, geometry=make_mesh.cpu())


def option_op(name: str, value: int) -> Op:
    def fn(mesh: Any, carried: Carried) -> dict:
        from pyapes_amd.hip.context import context_for
        ctx = context_for(mesh)
        ctx.set_option(name, value)
        carried.options[name] = value
        return {"set": value}
    return Op(f"set_option({name}, {value})", fn)


def apply_bcs_op(bcname: str, seed: int = 31) -> Op:
    """``Field.apply_bcs`` of a field of its own (between two solves of another)"""
    faces = BCSETS[bcname]

    def fn(mesh: Any, carried: Carried) -> dict:
        from pyapes_amd.variables import Field
        cfg, _, arrays = bc_configs(mesh, faces, None, seed)
        f = Field("q", 1, mesh, {"domain": cfg, "obstacle": None})
        f.set_var_tensor(_rand(mesh, seed).cuda())
        f.apply_bcs()
        out = {"q": f().cpu()}
        carried.own(f(), *arrays)
        return out

    def ref(before: Carried, out: dict, mesh: Any) -> None:
        import pyapes_oracle as O
        om = _omesh(mesh)
        _, ocfg, _ = bc_configs(mesh, faces, None, seed)
        want = O.bc_fill(_rand(mesh, seed), O.make_bcs(om, ocfg))
        assert torch.equal(out["q"], want), f"apply_bcs {bcname}"

    return Op(f"apply_bcs-{bcname}", fn, ref, pure=True)


def aop_op(bcname: str, seed: int = 41) -> Op:
    """``Solver.Aop`` and the rhs adjustment of an equation that is set but not solved"""
    faces = BCSETS[bcname]

    def fn(mesh: Any, carried: Carried) -> dict:
        from pyapes_amd.solver.fdm import FDM
        from pyapes_amd.solver.ops import Solver
        from pyapes_amd.variables import Field
        cfg, _, arrays = bc_configs(mesh, faces, None, seed)
        var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
        var.set_var_tensor(_rand(mesh, seed).cuda())
        var.apply_bcs()
        rhs_d = _rand(mesh, seed + 1).cuda()
        s = Solver({"fdm": {"method": "cg", "tol": -1.0, "max_it": 1, "report": False}})
        s.set_eq(-FDM().laplacian(0.7, var) == rhs_d)      # adjusts rhs_d in place
        ax = s.Aop(var)
        out = {"Ax": ax.cpu(), "rhs_adjusted": rhs_d.cpu()}
        carried.own(var(), rhs_d, ax, *arrays)
        return out

    def ref(before: Carried, out: dict, mesh: Any) -> None:
        import pyapes_oracle as O
        om = _omesh(mesh)
        _, ocfg, _ = bc_configs(mesh, faces, None, seed)
        obcs = O.make_bcs(om, ocfg)
        x = O.bc_fill(_rand(mesh, seed), obcs)
        want = O.Aop(x, [O.OTerm("laplacian", O.laplacian_tables(x, om, obcs), 0.7, -1.0)], om.dim)
        assert torch.equal(out["Ax"], want), ("Aop", float((out["Ax"] - want).abs().max()), int((out["Ax"] != want).sum()))
        want = _rand(mesh, seed + 1) + O.laplacian_rhs_adjust(x, om, obcs)
        assert torch.equal(out["rhs_adjusted"], want), ("rhs adjustment", float((out["rhs_adjusted"] - want).abs().max()))

    return Op(f"aop-{bcname}", fn, ref, pure=True)


# ---- explicit operators and marches ------------------------------------------------------------------------------------
MARCH_BC = ([0.5, 0.1, None, 1.0, -0.3, None], ["dirichlet", "neumann", "symmetry", "dirichlet", "neumann", "symmetry"])


def _march_setup(mesh: Any):
    """BC config of a scalar field, of a vector field (a value per component), their oracle lists, nu and dt"""
    import pyapes_oracle as O
    from pyapes_amd.variables.bcs import mixed_bcs
    nd = mesh.dim
    vals, types = MARCH_BC[0][:2 * nd], MARCH_BC[1][:2 * nd]
    om = _omesh(mesh)
    per_comp = [[None if v is None else v + 0.375 * c - 0.125 * f * c for f, v in enumerate(vals)] for c in range(nd)]
    bc_s = {"domain": mixed_bcs(list(vals), list(types)), "obstacle": None}
    bc_v = {"domain": mixed_bcs([None if vals[f] is None else [per_comp[c][f] for c in range(nd)] for f in range(2 * nd)], list(types)),
            "obstacle": None}
    obcs_s = O.make_bcs(om, O.mixed_cfg(vals, types, O.FACES[:2 * nd]))
    obcs_v = [O.make_bcs(om, O.mixed_cfg(per_comp[c], types, O.FACES[:2 * nd])) for c in range(nd)]
    dx = min(float(d) for d in mesh.dx_list)
    nu = 1e-3
    dt = 0.2 * min(dx * dx / (2 * nd * nu), dx / 1.3)
    return bc_s, bc_v, om, obcs_s, obcs_v, nu, dt


def start_op(seed: int = 5) -> Op:
    """the start of a time loop: a BC-filled vector field ``U``, a BC-filled scalar ``phi``, a zero pressure ``p``"""
    def fn(mesh: Any, carried: Carried) -> dict:
        import pyapes_oracle as O
        _, _, _, obcs_s, obcs_v, _, _ = _march_setup(mesh)
        U = 0.5 * _rand(mesh, seed, lead=mesh.dim)
        for c in range(mesh.dim):
            O.bc_fill(U[c:c + 1], obcs_v[c])
        phi = torch.rand(_rand(mesh, seed).shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64).to(U.dtype)
        O.bc_fill(phi, obcs_s)
        carried.fields.update(U=U, phi=phi, p=torch.zeros_like(phi))
        return {"U": U.clone(), "phi": phi.clone()}
    return Op("start", fn)


def march_op(kind: str, nsteps: int = 2, seed: int = 9) -> Op:
    """one entry point of solver/march.py on the carried fields.  kind: "momentum" (upwind, order 3), "quick3" (rk_march
    order 3, limiter quick, the speed a tensor), "minmod2" (order 2, limiter minmod, with source=), "euler" (euler_march,
    upwind, a scalar speed), "self" (rk_march(phi, phi), upwind, order 3)"""
    def speed_and_source(mesh: Any):
        return _rand(mesh, seed, scale=0.8), _rand(mesh, seed + 1, scale=3.0)

    def fn(mesh: Any, carried: Carried) -> dict:
        from pyapes_amd.solver import march as M
        from pyapes_amd.variables import Field
        bc_s, bc_v, _, _, _, nu, dt = _march_setup(mesh)
        u_c, s_c = speed_and_source(mesh)
        u_d, s_d = u_c.cuda(), s_c.cuda()
        if kind == "momentum":
            f = Field("U", mesh.dim, mesh, bc_v)
            f.set_var_tensor(carried.fields["U"].cuda())
            start = f()
            M.momentum_march(f, nu, dt, nsteps, {"div": {"limiter": "upwind"}}, order=3)
            carried.fields["U"] = f().cpu()
            carried.own(start, f())
            return {"U": f().cpu()}
        f = Field("phi", 1, mesh, bc_s)
        f.set_var_tensor(carried.fields["phi"].cuda())
        start = f()
        if kind == "quick3":
            M.rk_march(f, u_d, nu, dt, nsteps, {"div": {"limiter": "quick"}}, order=3)
        elif kind == "minmod2":
            M.rk_march(f, 0.7, nu, dt, nsteps, {"div": {"limiter": "minmod"}}, order=2, source=s_d)
        elif kind == "euler":
            M.euler_march(f, 0.7, nu, dt, nsteps + 1, {"div": {"limiter": "upwind"}})
        elif kind == "self":
            M.rk_march(f, f, nu, dt, nsteps, {"div": {"limiter": "upwind"}}, order=3)
        else:
            raise ValueError(kind)
        carried.fields["phi"] = f().cpu()
        carried.own(start, f(), u_d, s_d)
        return {"phi": f().cpu()}

    def ref(before: Carried, out: dict, mesh: Any) -> None:
        import march_ref as R
        _, _, om, obcs_s, obcs_v, nu, dt = _march_setup(mesh)
        u_c, s_c = speed_and_source(mesh)
        if kind == "momentum":
            want, got = R.momentum.march(before.fields["U"], nu, dt, nsteps, om, obcs_v, "upwind", 3), out["U"]
        else:
            phi = before.fields["phi"]
            got = out["phi"]
            if kind == "quick3":
                want = R.march(phi, u_c, nu, dt, nsteps, om, obcs_s, "quick", 3)
            elif kind == "minmod2":
                want = R.march(phi, 0.7, nu, dt, nsteps, om, obcs_s, "minmod", 2, s_c)
            elif kind == "euler":
                want = R.march(phi, 0.7, nu, dt, nsteps + 1, om, obcs_s, "upwind", 1)
            else:
                want = R.march(phi, None, nu, dt, nsteps, om, obcs_s, "upwind", 3, self_adv=True)
        assert torch.equal(got, want), (kind, float((got - want).abs().max()), int((got != want).sum()))

    return Op(f"march-{kind}", fn, ref)


def fdc_op(which: str) -> Op:
    """``FDC.grad`` of the carried pressure / ``FDC.laplacian`` of the carried scalar (edge False)"""
    def fn(mesh: Any, carried: Carried) -> dict:
        from pyapes_amd.solver.fdc import FDC
        from pyapes_amd.variables import Field
        bc_s = _march_setup(mesh)[0]
        f = Field("f", 1, mesh, bc_s)
        f.set_var_tensor(carried.fields["p" if which == "grad" else "phi"].cuda())
        fdc = FDC({"grad": {"edge": False}, "laplacian": {"edge": False}})
        res = fdc.grad(f) if which == "grad" else fdc.laplacian(f)
        out = {which: res.cpu()}
        carried.own(f(), res)
        return out

    def ref(before: Carried, out: dict, mesh: Any) -> None:
        import pyapes_oracle as O
        _, _, om, obcs_s, _, _, _ = _march_setup(mesh)
        x = before.fields["p" if which == "grad" else "phi"]
        if which == "grad":      # at EVERY node, like tests/test_gpu_unaligned.py (the carried fields are BC-filled)
            want = O.apply_grad(O.grad_tables(x, om, obcs_s), x, om.dim)[0]
            got = out["grad"][0]
        else:
            want = O.apply_laplacian(O.laplacian_tables(x, om, obcs_s), x, om.dim)
            got = out["laplacian"]
        assert got.shape == want.shape and torch.equal(got, want), (which, float((got - want).abs().max()), int((got != want).sum()))

    return Op(f"fdc-{which}", fn, ref)


def poisson_op(sweeps: int = 5) -> Op:
    """the pressure solve of the time loop: CG on ``-0.7 lap(p) = phi``, started from the carried ``p``"""
    return solve_op("cg", "dn", sweeps, carried_x="p", carried_rhs="phi", name=f"poisson-cg{sweeps}")


# ---- the stepwise CG -----------------------------------------------------------------------------------------------------
def stepwise_cg_op(bcname: str, iters: int, finish: bool, seed: int = 7) -> Op:
    """``cg_begin`` + ``cg_iterate(iters)`` + ``cg_end`` (finish) or ``cg_abort``"""
    faces = BCSETS[bcname]

    def fn(mesh: Any, carried: Carried) -> dict:
        from pyapes_amd.hip import lib as L
        from pyapes_amd.hip.context import context_for
        from pyapes_amd.variables import Field
        ctx = context_for(mesh)
        cfg, _, arrays = bc_configs(mesh, faces, None, seed)
        var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
        rhs_d = _rand(mesh, seed).cuda()
        ctx.bind_bcs(var(), var.bcs, 0, for_rhs=True)
        ctx.set_terms([{"kind": L.OP_LAPLACIAN, "sign": -1.0, "coeff": 0.7}])
        ctx.rhs_adjust(rhs_d[0])
        ctx.bind_bcs(var(), var.bcs, 0)
        ctx.cg_begin(var()[0], rhs_d[0], 1e-30, 1000)
        try:
            ctx.cg_iterate(iters)
            rep = ctx.cg_end() if finish else None
        finally:
            if not finish:
                ctx.cg_abort()
        carried.own(var(), rhs_d, *arrays)
        if not finish:
            return {"aborted": True}
        return {"x": var().cpu(), **_report(mesh, rep)}

    def ref(before: Carried, out: dict, mesh: Any) -> None:
        import pyapes_oracle as O
        if not finish:
            return
        _, ocfg, _ = bc_configs(mesh, faces, None, seed)
        xo, ro = _quiet(lambda: O.solve_poisson(_omesh(mesh), ocfg, _rand(mesh, seed), method="cg", tol=-1.0, max_it=iters - 1,
                                                coeff=0.7, sign=-1.0))
        assert out["itr"] == ro["itr"] == iters, (out["itr"], ro["itr"])
        assert _rel(out["x"], xo) < _bars(mesh), _rel(out["x"], xo)

    return Op(f"stepwise-cg{iters}-" + ("end" if finish else "abort"), fn, ref, pure=True)


def failing_solve_op(method: str = "cg") -> Op:
    """a right-hand side of inf: the library's ordinary PA_E_NONFINITE return, "Invalid tolerance" in Python"""
    def fn(mesh: Any, carried: Carried) -> dict:
        from pyapes_amd.solver.fdm import FDM
        from pyapes_amd.solver.ops import Solver
        from pyapes_amd.variables import Field
        cfg, _, _ = bc_configs(mesh, BCSETS["dir"], None, 0)
        var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
        rhs_d = torch.full((1, *[int(v) for v in mesh.nx]), float("inf"), dtype=mesh.dtype.float, device="cuda")
        s = Solver({"fdm": {"method": method, "tol": 1e-6, "max_it": 5, "report": False}})
        s.set_eq(FDM().laplacian(1.0, var) == rhs_d)
        try:
            _quiet(s.solve)
        except RuntimeError as e:
            carried.own(var(), rhs_d)
            return {"raised": "Invalid tolerance" in str(e)}
        return {"raised": False}

    def ref(before: Carried, out: dict, mesh: Any) -> None:
        assert out["raised"] is True

    return Op(f"nonfinite-{method}", fn, ref, pure=True)


# ---- axisymmetric meshes -------------------------------------------------------------------------------------------------
RZ_BC = ([0.0, 1.0, 0.3, 0.5], ["neumann", "dirichlet", "dirichlet", "neumann"])


def _rz_smooth(mesh: Any, seed: int) -> Tensor:
    """a smooth field on the (r, z) grid, (1, *n), CPU, in the mesh dtype"""
    om = _omesh(mesh)
    g = torch.Generator().manual_seed(seed)
    a, b, c = (float(v) for v in torch.rand(3, generator=g, dtype=torch.float64))
    r, z = om.grid[0].double(), om.grid[1].double()
    return (torch.exp(-(r - 0.3 - 0.2 * a) ** 2 / 0.1 - (z - 0.5 - 0.4 * b) ** 2 / 0.2) + 0.1 * c * r * z).unsqueeze(0).to(om.dtype)


def rz_operators_op(seed: int = 3) -> Op:
    """the operators of an axisymmetric mesh that read ``rz_tab``: FDC.laplacian and an Euler step (upwind, the u phi / r term)"""
    def fn(mesh: Any, carried: Carried) -> dict:
        import pyapes_oracle as O
        from pyapes_amd.solver.fdc import FDC
        from pyapes_amd.solver.march import euler_step
        from pyapes_amd.variables import Field
        om = _omesh(mesh)
        ocfg = O.mixed_cfg(*RZ_BC, O.FACES_RZ)
        pcfg = [dict(c, bc_val_opt=None) for c in ocfg]
        phi0 = O.bc_fill(_rz_smooth(mesh, seed), O.make_bcs(om, ocfg))
        f = Field("phi", 1, mesh, {"domain": pcfg, "obstacle": None})
        f.set_var_tensor(phi0.cuda())
        start = f()
        lap = FDC({"laplacian": {"edge": False}}).laplacian(f)
        euler_step(f, 0.8, 1e-2, 1e-3, {"div": {"limiter": "upwind"}})
        out = {"laplacian": lap.cpu(), "euler": f().cpu()}
        carried.own(start, f(), lap)
        return out

    def ref(before: Carried, out: dict, mesh: Any) -> None:
        import pyapes_oracle as O
        om = _omesh(mesh)
        obcs = O.make_bcs(om, O.mixed_cfg(*RZ_BC, O.FACES_RZ))
        phi0 = O.bc_fill(_rz_smooth(mesh, seed), obcs)
        lap = O.apply_laplacian(O.laplacian_tables(phi0, om, obcs), phi0, om.dim)
        assert torch.equal(out["laplacian"], lap), ("rz laplacian", float((out["laplacian"] - lap).abs().max()), int((out["laplacian"] != lap).sum()))
        want = O.euler_step(phi0.clone(), 0.8, 1e-2, 1e-3, om, obcs, "upwind")
        assert _rel(out["euler"], want) < (1e-13 if om.dtype == torch.float64 else 1e-6), _rel(out["euler"], want)

    return Op("rz-operators", fn, ref, pure=True)


def rz_solve_op(method: str, sweeps: int, seed: int = 2) -> Op:
    max_it = sweeps if method == "bicgstab" else sweeps - 1

    def fn(mesh: Any, carried: Carried) -> dict:
        import pyapes_oracle as O
        from pyapes_amd.solver.fdm import FDM
        from pyapes_amd.solver.ops import Solver
        from pyapes_amd.variables import Field
        pcfg = [dict(c, bc_val_opt=None) for c in O.mixed_cfg(*RZ_BC, O.FACES_RZ)]
        var = Field("p", 1, mesh, {"domain": pcfg, "obstacle": None})
        rhs_d = _rand(mesh, seed).cuda()
        s = Solver({"fdm": {"method": method, "tol": -1.0, "max_it": max_it, "report": False}})
        s.set_eq(FDM().laplacian(1.0, var) == rhs_d)
        rep = _quiet(s.solve)
        carried.own(var(), rhs_d)
        return {"x": var().cpu(), **_report(mesh, rep)}

    def ref(before: Carried, out: dict, mesh: Any) -> None:
        import pyapes_oracle as O
        xo, ro = _quiet(lambda: O.solve_poisson(_omesh(mesh), O.mixed_cfg(*RZ_BC, O.FACES_RZ), _rand(mesh, seed), method=method,
                                                tol=-1.0, max_it=max_it))
        assert out["itr"] == ro["itr"] == sweeps
        assert _rel(out["x"], xo) < _bars(mesh), _rel(out["x"], xo)

    return Op(f"rz-{method}{sweeps}", fn, ref, pure=True)


def rz_rfp_op(seed: int = 6) -> Op:
    """``RFP.friction`` / ``RFP.diffusion`` (the Rosenbluth-Fokker-Planck operators of an axisymmetric mesh)"""
    def fn(mesh: Any, carried: Carried) -> dict:
        from pyapes_amd.solver.fdc import hessian, jacobian
        from pyapes_amd.solver.rfp import RFP
        from pyapes_amd.variables import Field
        made = []

        def field(name: str, s: int):
            f = Field(name, 1, mesh, {"domain": None, "obstacle": None})
            f.set_var_tensor(_rz_smooth(mesh, s).cuda())
            made.append(f())
            return f
        pdf, H, G = field("pdf", seed), field("H", seed + 1), field("G", seed + 2)
        jacH, hessG = jacobian(H), hessian(G)
        rfp = RFP()
        fr, df = rfp.friction(jacH, pdf), rfp.diffusion(hessG, pdf)
        out = {"friction": fr.cpu(), "diffusion": df.cpu()}
        carried.own(*made, fr, df, jacH.r, jacH.z, hessG.rr, hessG.rz, hessG.zz)
        return out

    def ref(before: Carried, out: dict, mesh: Any) -> None:
        import pyapes_oracle as O
        om = _omesh(mesh)
        pdf, H, G = (_rz_smooth(mesh, seed + q)[0] for q in range(3))
        want_f = O.rfp_friction(O.jacobian(H, om), pdf, om)
        want_d = O.rfp_diffusion(O.hessian(G, om), pdf, om)
        assert torch.equal(out["friction"].reshape(want_f.shape), want_f), ("friction", float((out["friction"].reshape(want_f.shape) - want_f).abs().max()))
        assert torch.equal(out["diffusion"].reshape(want_d.shape), want_d), ("diffusion", float((out["diffusion"].reshape(want_d.shape) - want_d).abs().max()))

    return Op("rz-rfp", fn, ref, pure=True)


# ---- stepwise Jacobi on a slab mesh of one rank (spawned: the gloo process group of tests/test_gpu_slab.py) ----------------
def jacobi_parity_worker(rank: int, world: int, port: int, jobs: Sequence[tuple], out: str) -> None:
    """jobs: (key, n, dtype, options, K_first, K_second).  Per job, on ONE slab mesh: a SlabJacobi solve of K_first + 1 sweep
    launches, then one of K_second + 1; and the second solve alone on a FRESH mesh.  Records itr, tol, the stop-test sum and
    x of each."""
    import os
    import sys
    import torch.distributed as dist
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pyapes_amd.geometry import Box
        from pyapes_amd.hip.context import context_for
        from pyapes_amd.mesh import Mesh
        from pyapes_amd.slab import SlabJacobi
        from pyapes_amd.variables import Field
        torch.cuda.set_device(0)
        res = {}
        for key, n, dtype, opts, k_first, k_second in jobs:
            cfg = [{"bc_face": f, "bc_type": t, "bc_val": v, "bc_val_opt": None}
                   for f, (t, v) in zip(["xl", "xu", "yl", "yu", "zl", "zu"], BCSETS["mix"])]

            def solve(mesh, K, seed):
                var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
                rhs = torch.randn((1, *n), generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(mesh.dtype.float).cuda()
                drv = SlabJacobi(mesh, var, rhs, [{"kind": 0, "sign": -1.0, "coeff": 0.7}], dist, omega=0.9)
                rep = drv.solve(1e-30, K, poll=3)
                # sums[2]: the stop-test sum of the last executed sweep, before the square root that can hide its last bit
                return {"x": var().cpu(), "itr": int(rep.itr), "tol": float(rep.tol), "dx2": float(drv.sums[2])}

            def mesh_with_options():
                mesh = Mesh(Box[0:1, 0:1, 0:0.5], None, list(n), "cuda", dtype, slab=(rank, world))
                for k, v in opts.items():
                    context_for(mesh).set_option(k, v)
                return mesh

            used = mesh_with_options()
            first = solve(used, k_first, 7)
            second = solve(used, k_second, 8)
            fresh = solve(mesh_with_options(), k_second, 8)
            res[key] = {"first": first, "second": second, "fresh": fresh}
        if rank == 0:
            torch.save(res, out)
    finally:
        dist.destroy_process_group()
