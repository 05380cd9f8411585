"""What the -m gpu tests of the explicit marches share, statement for statement: the child process with the launch log on and
the parser of its log, the BC tables and mesh lists, the Div kind / config of a limiter name, a fresh Field, the march composed
of single launches, and the seed-5 inputs of tests/test_gpu_source.py and tests/test_gpu_velocity.py.  A plain module: no test
lives here, and whatever exists once stays in its test file.
"""
import ctypes as C
import os
import subprocess
import sys

import torch

import pyapes_oracle as O
from pyapes_amd.geometry import Box
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdc import div_kind
from pyapes_amd.solver.march import SSP_STAGES
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

ALLDIR = ([0.0, 1.0, 0.25, -0.5, 2.0, 0.0], ["dirichlet"] * 6)
MIXED = ([0.5, 0.1, None, 1.0, -0.3, None], ["dirichlet", "neumann", "symmetry", "dirichlet", "neumann", "symmetry"])
XPER = ([None, None, 0.25, -0.5, 2.0, 0.0], ["periodic", "periodic", "dirichlet", "dirichlet", "dirichlet", "dirichlet"])
BCS = {"dir": ALLDIR, "mix": MIXED, "xper": XPER}
ZPER = ([0.25, -0.5, 2.0, 0.0, None, None], ["dirichlet", "dirichlet", "dirichlet", "dirichlet", "periodic", "periodic"])   # beside BCS
LIMITER_BCS = {"upwind": ("dir", "mix"), "quick": ("dir", "mix"), "none": ("dir",),   # central Div refuses neumann / symmetry
               "minmod": ("dir", "mix"), "mc": ("dir", "mix")}

VECTOR = [([7, 13, 132], "double"), ([9, 14, 132], "double"), ([7, 13, 260], "single"), ([9, 14, 260], "single")]
GENERIC = [([6, 7, 9], "double"), ([17, 12], "double"), ([33], "single")]
VECTOR_OPTIONS = [{"sf": sf, "chunks": ch} for sf in (2, 4) for ch in (1, 2, 3)]


def mesh_id(v):
    """the parametrize id of an (n, dtype) pair's members"""
    return "x".join(map(str, v)) if isinstance(v, list) else v


def box(nd):
    return Box[0:1] if nd == 1 else (Box[0:1, 0:1] if nd == 2 else Box[0:1, 0:1, 0:1])


def kind(limiter):
    """the Div kind of a limiter name of tests/march_ref.py ("compat": the literal upwind form)"""
    return div_kind("upwind" if limiter == "compat" else limiter, limiter == "compat")


def config(limiter):
    return {"div": {"limiter": "upwind" if limiter == "compat" else limiter, "compat": limiter == "compat"}}


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def fresh_field(mesh, bc, t, time=False):
    """a new Field of ``t.shape[0]`` components holding a device copy of ``t``"""
    f = Field("phi", t.shape[0], mesh, bc)
    f.set_var_tensor(t.to("cuda", copy=True))
    if time:
        f.set_time(0.0, 1.5)
    return f


def child(code, drop_options=False):
    """``code`` in a fresh python process with the launch log on (PYAPES_HIP_DEBUG); returns its stderr"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pre = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (root, os.path.join(root, "tests"))
    env = dict(os.environ, PYAPES_HIP_DEBUG="1",
               PYTHONPATH=os.pathsep.join([os.path.join(root, "oracle"), os.environ.get("PYTHONPATH", "")]))
    if drop_options:
        env.pop("PYAPES_HIP_OPTIONS", None)
    r = subprocess.run([sys.executable, "-c", pre + code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def case_log(log, keep):
    """{case: [the lines behind its ``CASE <case>`` marker that ``keep`` accepts]}.  The launch log is limited per kernel
    instantiation, so a child prints a marker in front of every case and only the lines behind it are read."""
    seen, cur = {}, None
    for ln in log.splitlines():
        if ln.startswith("CASE "):
            cur = ln[5:].strip()
            seen[cur] = []
        elif cur is not None and keep(ln):
            seen[cur].append(ln)
    return seen


def march_by_stages(step, stage, phi, order, nsteps):
    """the march composed of single launches: ``step(phi0)`` is the Euler step of a copy of the step's start, and
    ``stage(cur, phi0, c0, c1)`` the stage B(c0 phi0 + c1 E(cur)); both return a new tensor"""
    for _ in range(nsteps):
        phi0 = phi.clone()
        cur = step(phi0)
        for c0, c1 in SSP_STAGES[order]:
            cur = stage(cur, phi0, c0, c1)
        phi = cur
    return phi


_SETUPS = {}


def setup(n, dtype, bcname, lead):
    """the GPU mesh and BC config, the oracle's mesh and BCs, and CPU tensors from seed 5: two BC-filled fields, a speed
    (lead, *n) -- one speed field, or a velocity with distinct random components -- and a source; nu and dt"""
    key = (tuple(n), dtype, bcname, lead)
    if key not in _SETUPS:
        nd = len(n)
        vals, types = BCS[bcname]
        vals, types = vals[:2 * nd], types[:2 * nd]
        mesh = Mesh(box(nd), None, list(n), "cuda", dtype)
        bc = {"domain": mixed_bcs(vals, types), "obstacle": None}
        om = O.OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
        obcs = O.make_bcs(om, O.mixed_cfg(vals, types, O.FACES[:2 * nd]))
        g = torch.Generator().manual_seed(5)
        tdt = mesh.dtype.float
        fields = []
        for _ in range(2):
            t = torch.rand((1, *n), generator=g, dtype=torch.float64).to(tdt)
            O.bc_fill(t, obcs)
            fields.append(t)
        speed = torch.randn((lead, *n), generator=g, dtype=torch.float64).to(tdt)
        src = (3.0 * torch.randn((1, *n), generator=g, dtype=torch.float64)).to(tdt)
        dx = min(float(d) for d in mesh.dx_list)
        nu = 1e-3
        dt = 0.2 * min(dx * dx / (2 * nd * nu), dx / 1.3)
        _SETUPS[key] = (mesh, bc, om, obcs, fields[0], fields[1], speed, src, nu, dt)
    return _SETUPS[key]
