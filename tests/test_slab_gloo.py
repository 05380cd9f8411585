"""CPU, world_size 2, gloo: the slab driver (pyapes_amd/slab.py: halo exchange of r planes, ring
wrap, periodic far planes, scalar all-reduces, phase order) with the torch stand-in backend,
against the single-domain oracle.  Also the host-side partitioning logic."""
import os
import socket
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pyapes_oracle as O
from pyapes_amd.slab import slab_extent

D = lambda v=0.0: ("dirichlet", v)   # noqa: E731
N = lambda v=0.0: ("neumann", v)     # noqa: E731
SY = ("symmetry", None)
PE = ("periodic", None)
CASES = {
    "dir": [D(0.0), D(0.5), D(0.0), D(0.0), D(1.0), D(0.0)],
    "mix": [N(0.3), D(0.0), D(0.3), N(0.0), SY, N(-0.25)],
    "neu_hi": [D(0.2), N(0.0), SY, SY, D(1.0), D(0.0)],
    "per": [PE] * 6,
    "xper": [PE, PE, D(0.0), D(1.0), N(0.0), SY],
}


def test_slab_extent_partitions_exactly():
    for n0 in (6, 7, 12, 512, 1024, 33):
        for world in (1, 2, 3, 4, 8):
            if n0 < 3 * world:
                with pytest.raises(ValueError):
                    slab_extent(n0, 0, world)
                continue
            ext = [slab_extent(n0, r, world) for r in range(world)]
            assert ext[0][0] == 0 and sum(e[1] for e in ext) == n0
            for a, b in zip(ext, ext[1:]):
                assert a[0] + a[1] == b[0]
            assert max(e[1] for e in ext) - min(e[1] for e in ext) <= 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(fn, args_of_port, nprocs):
    """mp.spawn with a fresh rendezvous port; a port that was free when looked up can be taken by the time the
    TCPStore listens on it (many spawns in a row): try again with another one instead of failing the test."""
    for attempt in range(4):
        try:
            mp.spawn(fn, args=args_of_port(_free_port()), nprocs=nprocs, join=True)
            return
        except Exception as e:   # ProcessRaisedException carries the child's traceback as text
            if "EADDRINUSE" in str(e) and attempt < 3:
                continue
            raise


class _FailingOnce:
    """The stand-in backend, raising once in the ``fail_at``-th phase B (the same step on every rank, so no rank is left
    waiting in a collective) and recording the calls that clean up after it."""

    def __init__(self, be, fail_at):
        self.be, self.fail_at, self.n_b, self.calls = be, fail_at, 0, []

    def __getattr__(self, name):
        return getattr(self.be, name)

    def cg_phase_b(self):
        self.n_b += 1
        if self.n_b == self.fail_at:
            raise RuntimeError("injected failure in phase B")
        return self.be.cg_phase_b()

    def cg_abort(self):
        self.calls.append("cg_abort")
        return self.be.cg_abort()

    def slab_set(self, bufs):
        self.calls.append("slab_set" if bufs is not None else "slab_set(None)")
        return self.be.slab_set(bufs)


def _worker(rank, world, port, name, n, K, dtype, out, fail_at=0):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    warnings.filterwarnings("ignore")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pyapes_amd.geometry import Box
        from pyapes_amd.mesh import Mesh
        from pyapes_amd.slab import SlabCG
        from pyapes_amd.variables import Field
        from slab_torch_backend import TorchSlabBackend
        bcs = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v, "bc_val_opt": None}
               for i, (t, v) in enumerate(CASES[name])]
        mesh = Mesh(Box[0:1, 0:1, 0:0.5], None, list(n), "cpu", dtype, slab=(rank, world))
        var = Field("p", 1, mesh, {"domain": bcs, "obstacle": None})
        g = torch.Generator().manual_seed(7)
        rhs_g = torch.randn((1, *n), generator=g, dtype=torch.float64).to(mesh.dtype.float)
        if name == "per":
            rhs_g -= rhs_g.mean()
        rhs = rhs_g[:, mesh.i_off:mesh.i_off + mesh.nx[0]].clone()
        be = TorchSlabBackend(mesh)
        drv = SlabCG(mesh, var, rhs, [{"kind": 0, "sign": -1.0, "coeff": 0.7}], dist, backend=be)
        if fail_at:
            be = _FailingOnce(be, fail_at)
            drv.be = be
            x0, rhs0 = var().clone(), rhs.clone()
            with pytest.raises(RuntimeError, match="injected"):
                drv.solve(1e-30, K, poll=3)
            assert be.calls[-2:] == ["cg_abort", "slab_set(None)"], be.calls[-4:]
            var()[:] = x0                   # the same start for the second solve on this driver and mesh
            rhs[:] = rhs0
        rep = drv.solve(1e-30, K, poll=3)
        parts = [None] * world
        dist.all_gather_object(parts, var().clone())
        if rank == 0:
            torch.save({"x": torch.cat(parts, dim=1), "itr": rep.itr, "tol": rep.tol}, out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name,fail_at", [(c, 0) for c in CASES] + [("mix", 4)], ids=list(CASES) + ["mix-after-error"])
def test_slab_driver_two_ranks_matches_oracle(name, fail_at, tmp_path):
    """(mix-after-error: a solve that raises inside ``iterate`` drops the live solve and leaves slab mode; the next
    solve on the same driver and mesh runs as if it had not happened)"""
    n, K, dtype = (12, 9, 10), 7, "double"
    out = str(tmp_path / "x.pt")
    spawn_ranks(_worker, lambda port: (2, port, name, n, K, dtype, out, fail_at), 2)
    res = torch.load(out)
    mesh = O.OMesh([0, 0, 0], [1, 1, 0.5], list(n), dtype)
    cfg = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(CASES[name])]
    g = torch.Generator().manual_seed(7)
    rhs = torch.randn((1, *n), generator=g, dtype=torch.float64)
    if name == "per":
        rhs -= rhs.mean()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xo, ro = O.solve_poisson(mesh, cfg, rhs, method="cg", tol=1e-30, max_it=K, coeff=0.7, sign=-1.0)
    assert res["itr"] == ro["itr"] == K + 1
    err = float(torch.linalg.norm(res["x"] - xo) / torch.linalg.norm(xo))
    assert err < 1e-12, err
    assert abs(res["tol"] - ro["tol"]) <= 1e-10 * abs(ro["tol"])


# ---- Solver.solve() on a slab mesh: the reference's own surface (ops.py:92-109) ends in the slab drivers ---------------
def _worker_solve(rank, world, port, name, n, K, method, tol, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    warnings.filterwarnings("ignore")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pyapes_amd.geometry import Box
        from pyapes_amd.mesh import Mesh
        from pyapes_amd.solver.fdm import FDM
        from pyapes_amd.solver.ops import Solver
        from pyapes_amd.variables import Field
        from slab_torch_backend import TorchSlabBackend
        bcs = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v, "bc_val_opt": None}
               for i, (t, v) in enumerate(CASES[name])]
        mesh = Mesh(Box[0:1, 0:1, 0:0.5], None, list(n), "cpu", "double", slab=(rank, world))
        mesh._hip = TorchSlabBackend(mesh)          # the torch stand-in for the C calls (context_for(mesh) returns it)
        var = Field("p", 1, mesh, {"domain": bcs, "obstacle": None})
        g = torch.Generator().manual_seed(7)
        rhs_g = torch.randn((1, *n), generator=g, dtype=torch.float64)
        if name == "per":
            rhs_g -= rhs_g.mean()
        rhs = rhs_g[:, mesh.i_off:mesh.i_off + mesh.nx[0]].clone()
        cfg = {"method": method, "tol": tol, "max_it": K, "report": False}
        if method == "jacobi":
            cfg["omega"] = 0.9
        solver = Solver({"fdm": cfg})
        solver.set_eq(-FDM().laplacian(0.7, var) == rhs)        # rhs adjustment: rank-local
        rep = solver.solve()
        parts = [None] * world
        dist.all_gather_object(parts, var().clone())
        if rank == 0:
            torch.save({"x": torch.cat(parts, dim=1), "itr": rep["itr"], "tol": rep["tol"], "converge": rep["converge"]}, out)
    finally:
        dist.destroy_process_group()


def _oracle_solve(name, n, K, method, tol):
    mesh = O.OMesh([0, 0, 0], [1, 1, 0.5], list(n), "double")
    cfg = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(CASES[name])]
    g = torch.Generator().manual_seed(7)
    rhs = torch.randn((1, *n), generator=g, dtype=torch.float64)
    if name == "per":
        rhs -= rhs.mean()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kw = {"omega": 0.9} if method == "jacobi" else {}
        return O.solve_poisson(mesh, cfg, rhs, method=method, tol=tol, max_it=K, coeff=0.7, sign=-1.0, **kw)


@pytest.mark.parametrize("method", ["cg", "bicgstab", "jacobi"])
@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_solver_solve_on_a_slab_mesh_two_ranks(name, method, tmp_path):
    """``Solver.set_eq() / solve()`` with ``Mesh(..., slab=(rank, 2))`` on both ranks: linalg.solve dispatches to the slab
    driver (CG: SlabCG, BiCGSTAB: SlabBiCGSTAB, Jacobi: SlabJacobi) -- the reference's surface, identical iteration counts, <= 1e-10 against
    the single-domain oracle."""
    n, K = (12, 9, 10), 7
    out = str(tmp_path / "x.pt")
    spawn_ranks(_worker_solve, lambda port: (2, port, name, n, K, method, 1e-30, out), 2)
    res = torch.load(out)
    xo, ro = _oracle_solve(name, n, K, method, 1e-30)
    assert res["itr"] == ro["itr"] == (K if method == "bicgstab" else K + 1)
    assert res["converge"] == ro["converge"]
    err = float(torch.linalg.norm(res["x"] - xo) / torch.linalg.norm(xo))
    assert err < 1e-10, err
    assert abs(res["tol"] - ro["tol"]) <= 1e-8 * abs(ro["tol"])


def test_slab_bicgstab_converges_where_periodic_cg_cannot(tmp_path):
    """SURVEY Q5 on two ranks: with a periodic axis CG never meets the reference's stop test (the BC fill keeps moving the
    boundary nodes), BiCGSTAB -- residual-based -- converges.  Axis 0 periodic = the ring across the ranks."""
    n, K = (12, 9, 10), 400
    out = str(tmp_path / "x.pt")
    spawn_ranks(_worker_solve, lambda port: (2, port, "xper", n, K, "bicgstab", 1e-9, out), 2)
    res = torch.load(out)
    xo, ro = _oracle_solve("xper", n, K, "bicgstab", 1e-9)
    assert res["converge"] and ro["converge"]
    # (the count of such a run is summation-order sensitive -- the reference algorithm itself moves by tens of iterations
    # when only the order of its torch.sum changes, DESIGN 5 -- and two ranks add in another order than one domain)
    assert 0.5 * ro["itr"] <= res["itr"] <= 2 * ro["itr"], (res["itr"], ro["itr"])
    assert res["tol"] <= 1e-9 and ro["tol"] <= 1e-9
    err = float(torch.linalg.norm(res["x"] - xo) / torch.linalg.norm(xo))
    assert err < 1e-6, err


# ---- the explicit Euler march on slab meshes (solver/march.py -> slab.SlabEuler) -------------------------------------------
def _worker_euler(rank, world, port, name, n, nsteps, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    warnings.filterwarnings("ignore")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pyapes_amd.geometry import Box
        from pyapes_amd.mesh import Mesh
        from pyapes_amd.solver.march import euler_march
        from pyapes_amd.variables import Field
        from slab_torch_backend import TorchSlabBackend
        bcs = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v, "bc_val_opt": None}
               for i, (t, v) in enumerate(CASES[name])]
        mesh = Mesh(Box[0:1, 0:1, 0:0.5], None, list(n), "cpu", "double", slab=(rank, world))
        mesh._hip = TorchSlabBackend(mesh)
        phi = Field("phi", 1, mesh, {"domain": bcs, "obstacle": None})
        phi.set_var_tensor(euler_start(name, n)[:, mesh.i_off:mesh.i_off + mesh.nx[0]].clone())
        euler_march(phi, EULER_U, EULER_NU, EULER_DT, nsteps)
        parts = [None] * world
        dist.all_gather_object(parts, phi().clone())
        if rank == 0:
            torch.save({"x": torch.cat(parts, dim=1)}, out)
    finally:
        dist.destroy_process_group()


EULER_U, EULER_NU, EULER_DT = 0.8, 0.05, 2e-4


def euler_start(name, n, dtype="double"):
    """A BC-filled start field (the march assumes one, like the single-GPU march)."""
    mesh = O.OMesh([0, 0, 0], [1, 1, 0.5], list(n), dtype)
    cfg = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(CASES[name])]
    g = torch.Generator().manual_seed(11)
    phi = torch.randn((1, *n), generator=g, dtype=torch.float64).to(mesh.dtype)
    return O.bc_fill(phi, O.make_bcs(mesh, cfg))


def euler_oracle(name, n, nsteps, dtype="double"):
    mesh = O.OMesh([0, 0, 0], [1, 1, 0.5], list(n), dtype)
    cfg = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(CASES[name])]
    bcs = O.make_bcs(mesh, cfg)
    phi = euler_start(name, n, dtype)
    for _ in range(nsteps):
        phi = O.euler_step(phi, EULER_U, EULER_NU, EULER_DT, mesh, bcs)
    return phi


@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_euler_march_on_a_slab_mesh_two_ranks(name, tmp_path):
    """``euler_march`` with ``Mesh(..., slab=(rank, 2))`` on both ranks (SlabEuler: ghost planes of phi in, step, the far
    planes of the new field across a periodic ring, BC fill), odd number of steps, against the single-domain oracle."""
    n, nsteps = (12, 9, 10), 5
    out = str(tmp_path / "x.pt")
    spawn_ranks(_worker_euler, lambda port: (2, port, name, n, nsteps, out), 2)
    res = torch.load(out)
    xo = euler_oracle(name, n, nsteps)
    err = float(torch.linalg.norm(res["x"] - xo) / torch.linalg.norm(xo))
    assert err < 1e-12, err
