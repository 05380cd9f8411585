"""What the -m gpu tests of the projection layer share (tests/test_gpu_projection.py, tests/test_gpu_pressure.py): the BC sets,
scales and meshes, the seeded inputs of the kernel tests, a device copy off 16-byte alignment, and the walled / periodic case
of the ``project`` / ``ns_step`` tests.  A plain module like march_gpu.py: no test lives here.
"""
import torch

import march_gpu as G
import pyapes_oracle as O
from grid_cap_cases import MESHES, PASS, cells
from helpers import offset_view
from march_gpu import ALLDIR, MIXED, XPER
from pyapes_amd.mesh import Mesh
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

BCS = {"dir": ALLDIR, "mix": MIXED, "xper": XPER, "per": ([None] * 6, ["periodic"] * 6)}
TWO_PASSES = MESHES["one_and_a_bit"][0]
assert PASS < cells(TWO_PASSES) < 1.02 * PASS
DT = 0.003
SCALES = (1.0, 1.0 / DT, -0.75)

_SETUPS = {}


def setup(n, dtype, bcname):
    """the GPU mesh and its BC config (one type per face, a value per component), the oracle mesh and BC list (its values
    are lists: one per component), and CPU tensors: a BC-filled vector field with distinct random components and a scalar
    (seed 5), and, distinct from both, an increment and a right-hand side (1, *n) (seed 17, the same under every BC set)"""
    key = (tuple(n), dtype, bcname)
    if key not in _SETUPS:
        nd = len(n)
        vals, types = BCS[bcname]
        vals, types = vals[:2 * nd], types[:2 * nd]
        per_face = [None if v is None else [v + 0.375 * c - 0.125 * f * c for c in range(nd)] for f, v in enumerate(vals)]
        mesh = Mesh(G.box(nd), None, list(n), "cuda", dtype)
        bc = {"domain": mixed_bcs(per_face, types), "obstacle": None}
        om = O.OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
        obcs = O.make_bcs(om, O.mixed_cfg(per_face, types, O.FACES[:2 * nd]))
        g, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(17)
        tdt = mesh.dtype.float
        U = torch.randn((nd, *n), generator=g, dtype=torch.float64).to(tdt)
        O.bc_fill(U, obcs)
        p = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
        phi, nrhs = (torch.randn((1, *n), generator=g2, dtype=torch.float64).to(tdt) for _ in range(2))
        _SETUPS[key] = (mesh, bc, om, obcs, U, p, phi, nrhs)
    return _SETUPS[key]


def dev(t, k):
    """a device copy of ``t``: plain (k None), or a view ``k`` elements off a 16-byte boundary with guards (helpers.offset_view)"""
    if k is None:
        return t.cuda(), None
    return offset_view(t.cuda(), k)


def project_case(kind, dtype):
    """the mesh, oracle mesh, BC configs and lists, and CPU tensors U (3, *n) and p (1, *n) of the ``project`` / ``ns_step`` tests"""
    if kind == "periodic":
        n = [16, 16, 32]
        utypes, uvals = ["periodic"] * 6, [None] * 6
        ptypes, pvals = ["periodic"] * 6, [None] * 6
    else:   # walls, a lid on zu, an outflow face xu: U leaves it freely (neumann 0), p = 0 there makes the system non-singular
        n = [12, 20, 36]
        utypes = ["dirichlet", "neumann", "dirichlet", "dirichlet", "dirichlet", "dirichlet"]
        uvals = [[0.3, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.5, 0.0]]
        ptypes = ["neumann", "dirichlet", "neumann", "neumann", "neumann", "neumann"]
        pvals = [0.0] * 6
    mesh = Mesh(G.box(3), None, n, "cuda", dtype)
    om = O.OMesh([0.0] * 3, [1.0] * 3, n, dtype)
    ubc = {"domain": mixed_bcs(uvals, utypes), "obstacle": None}
    pbc = {"domain": mixed_bcs(pvals, ptypes), "obstacle": None}
    ubcs = O.make_bcs(om, O.mixed_cfg(uvals, utypes))
    pcfg = O.mixed_cfg(pvals, ptypes)
    g = torch.Generator().manual_seed(9)
    X = [x.double() for x in om.grid]
    U = torch.stack([torch.sin(2.0 * X[0] + 0.3) * torch.cos(3.0 * X[1]) + 0.2 * X[2],
                     torch.cos(1.5 * X[1] - 0.2) * torch.sin(2.5 * X[2]) - 0.1 * X[0],
                     torch.sin(3.0 * X[2] + 0.1) * torch.cos(2.0 * X[0]) + 0.3 * X[1]])
    U = (U + 0.05 * torch.randn(U.shape, generator=g, dtype=torch.float64)).to(om.dtype)
    p = (0.01 * torch.randn((1, *n), generator=g, dtype=torch.float64)).to(om.dtype)
    return mesh, om, ubc, pbc, ubcs, pcfg, U, p


def pressure(mesh, pbc, p_c):
    pf = Field("p", 1, mesh, pbc)
    pf.set_var_tensor(p_c.cuda())
    return pf
