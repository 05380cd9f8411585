"""The argument checks of the fourteen explicit-march entry points of the C ABI, called through ``lib`` directly: which
calls are refused, with which return code and which message -- and, where one call breaks two rules, WHICH rule answers.
Every bad call is refused before anything is enqueued.  Then the order-1 marches: two buffers ping-pong, ``w2`` is not
touched, ``*final == nsteps & 1`` and the result is ``nsteps`` calls of the matching single-step entry, bit for bit.
"""
import ctypes as C

import pytest
import torch

from pyapes_amd.geometry import Box
from pyapes_amd.hip import lib as L
from pyapes_amd.hip.context import context_for
from pyapes_amd.mesh import Mesh
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

UPWIND, COMPAT, BADKIND = L.OP_DIV_UPWIND, L.OP_DIV_UPWIND_COMPAT, 99
NU, DT = 1e-3, 1e-3
ARG = L.PA_E_ARG

# argument lists, in the order of include/pyapes_hip.h (after the context)
_ONE = ["kind", "u", "uf", "nu", "dt"]
ENTRIES = {
    "pa_euler_step": ["a", "b", *_ONE],
    "pa_euler_step_src": ["a", "b", *_ONE, "src"],
    "pa_euler_march": ["a", "b", *_ONE, "nsteps"],
    "pa_euler_march_src": ["a", "b", *_ONE, "nsteps", "src"],
    "pa_rk_stage": ["a", "p0", "o", "c0", "c1", *_ONE],
    "pa_rk_stage_src": ["a", "p0", "o", "c0", "c1", *_ONE, "src"],
    "pa_rk_march": ["a", "b", "c", "order", *_ONE, "nsteps", "final"],
    "pa_rk_march_src": ["a", "b", "c", "order", *_ONE, "nsteps", "final", "src"],
    "pa_rk_march_self": ["a", "b", "c", "order", "kind", "nu", "dt", "nsteps", "final"],
    "pa_rk_march_self_src": ["a", "b", "c", "order", "kind", "nu", "dt", "nsteps", "final", "src"],
    "pa_euler_step_vel": ["a", "b", "kind", "vel", "nu", "dt", "src"],
    "pa_rk_stage_vel": ["a", "p0", "o", "c0", "c1", "kind", "vel", "nu", "dt", "src"],
    "pa_rk_march_vel": ["a", "b", "c", "order", "kind", "vel", "nu", "dt", "nsteps", "final", "src"],
    "pa_momentum_march": ["A", "B", "Cc", "ncomp", "order", "kind", "frozen", "nu", "dt", "nsteps", "final", "srcs", "bcv"],
}
BUFFERS = ("a", "b", "c", "p0", "o", "uf", "A", "B", "Cc")


class Env:
    """one mesh, its context with an all-dirichlet BC list bound, and the buffers a call may name"""

    def __init__(self, n):
        nd = len(n)
        box = Box[0:1, 0:1] if nd == 2 else Box[0:1, 0:1, 0:1]
        self.mesh = Mesh(box, None, list(n), "cuda", "double")
        vals = [0.0, 1.0, 0.25, -0.5, 2.0, 0.0][:2 * nd]
        bc = {"domain": mixed_bcs(vals, ["dirichlet"] * (2 * nd)), "obstacle": None}
        self.ctx = context_for(self.mesh)
        f = Field("phi", 1, self.mesh, bc)
        self.ctx.bind_bcs(f(), f.bcs, 0)
        self.lib, self.h = self.ctx.lib, self.ctx.h
        g = torch.Generator().manual_seed(3)
        self.t = {k: torch.rand(tuple(n), generator=g, dtype=torch.float64).cuda() for k in ("a", "b", "c", "p0", "o", "x", "y")}
        self.ctx.apply_bc_bound(self.t["a"])
        vec = torch.rand((4 * 3, *n), generator=g, dtype=torch.float64).cuda()   # room for three (3, *n) vectors and one spare
        self.t.update(A=vec[0:3], B=vec[3:6], Cc=vec[6:9], X=vec[9:12],
                      AB=vec[1:4])   # a (3, *n) vector that overlaps A and B
        self.final = C.c_int(-7)
        self.bcv = (L.PaBcValues * 3)()

    def ptr(self, v):
        if v is None:
            return None
        return C.c_void_p((self.t[v] if isinstance(v, str) else v).data_ptr())

    def source(self, v):
        """None; ("field", name): that buffer as the source field; a float: the scalar source"""
        if v is None:
            return None
        s = L.PaSource()
        s.has = 1
        if isinstance(v, tuple):
            s.field = self.t[v[1]].data_ptr()
        else:
            s.value = float(v)
        return s

    def velocity(self, v):
        """None; "good": three scalars; "off": has == 0; ("field", name): axis 1's speed is that buffer"""
        if v is None:
            return None
        pv = L.PaVelocity()
        pv.has = 0 if v == "off" else 1
        pv.value[0], pv.value[1], pv.value[2] = 0.9, -0.4, 0.3
        if isinstance(v, tuple):
            pv.field[1] = self.t[v[1]].data_ptr()
        return pv

    def call(self, name, **over):
        d = dict(a="a", b="b", c="c", p0="p0", o="o", A="A", B="B", Cc="Cc", uf=None, kind=UPWIND, u=0.9, nu=NU, dt=DT,
                 c0=0.75, c1=0.25, order=2, nsteps=1, final="yes", src=None, vel="good", frozen=None, srcs=None,
                 ncomp=self.mesh.dim, bcv="yes")
        d.update(over)
        self.final.value = -7
        keep = []
        args = []
        for p in ENTRIES[name]:
            v = d[p]
            if p in BUFFERS:
                v = self.ptr(v)
            elif p == "final":
                v = None if v is None else C.byref(self.final)
            elif p == "bcv":
                v = None if v is None else self.bcv
            elif p == "src":
                v = self.source(v)
                keep.append(v)
                v = None if v is None else C.byref(v)
            elif p in ("vel", "frozen"):
                v = self.velocity(v)
                keep.append(v)
                v = None if v is None else C.byref(v)
            elif p == "srcs":
                if v is not None:
                    arr = (L.PaSource * 3)()
                    one = self.source(v)
                    arr[1].has, arr[1].value, arr[1].field = one.has, one.value, one.field
                    v = arr
            args.append(v)
        rc = getattr(self.lib, name)(self.h, *args)
        return rc, self.lib.pa_last_error(self.h).decode()


_ENVS = {}


def _env(n):
    if tuple(n) not in _ENVS:
        _ENVS[tuple(n)] = Env(n)
    return _ENVS[tuple(n)]


def _cases():
    """(entry, overrides, return code, a word of the message or None) -- every expected value read off the code as it was
    before the march layer was unified"""
    out = []

    def add(name, rc, word, **over):
        out.append(pytest.param(name, over, rc, word, id=f"{name}-{'-'.join(f'{k}={v}' for k, v in over.items())}"))

    # single steps
    for name in ("pa_euler_step", "pa_euler_step_src", "pa_euler_step_vel"):
        add(name, ARG, "in-place", b="a")
        add(name, ARG, "bad div kind", b="a", kind=BADKIND)            # the kind is looked at first
    for name in ("pa_euler_step_src", "pa_euler_step_vel"):
        add(name, ARG, "source field", src=("field", "a"))
        add(name, ARG, "source field", src=("field", "b"))
        add(name, ARG, "in-place", b="a", src=("field", "a"))          # the buffers before the source
    add("pa_euler_step_src", ARG, "source field", uf="x", src=("field", "x"))
    # stages
    for name in ("pa_rk_stage", "pa_rk_stage_src", "pa_rk_stage_vel"):
        add(name, ARG, "buffer of its own", o="a")
        add(name, ARG, "buffer of its own", o="p0")
        add(name, ARG, "bad div kind", o="a", kind=BADKIND)
    for name in ("pa_rk_stage_src", "pa_rk_stage_vel"):
        add(name, ARG, "source field", src=("field", "p0"))
        add(name, ARG, "source field", src=("field", "o"))
    # the velocity of a step / stage / march
    for name in ("pa_euler_step_vel", "pa_rk_stage_vel", "pa_rk_march_vel"):
        add(name, ARG, "velocity is needed", vel="off")
        add(name, ARG, "velocity is needed", vel=None)
        add(name, ARG, "literal upwind", kind=COMPAT)
        add(name, ARG, "velocity is needed", vel="off", kind=COMPAT)   # has == 0 before the kind
        add(name, ARG, "velocity field", vel=("field", "x"), src=("field", "x"))
        add(name, ARG, "velocity field", vel=("field", "a"))
        add(name, ARG, "source field", vel="off", src=("field", "a"))  # the source before the velocity
    # the Euler march
    for name in ("pa_euler_march", "pa_euler_march_src"):
        add(name, ARG, "bad buffers", b="a")
        add(name, ARG, "bad buffers", nsteps=-1)
        add(name, ARG, "bad div kind", b="a", kind=BADKIND)
    add("pa_euler_march_src", ARG, "source field", src=("field", "b"))
    add("pa_euler_march_src", ARG, "source field", uf="x", src=("field", "x"))
    # the Runge-Kutta marches: pa_rk_march(_src) wants three buffers at every order, the others two at order 1
    three, two = "three distinct buffers", "two for order 1, else three"
    for name in ("pa_rk_march", "pa_rk_march_src", "pa_rk_march_self", "pa_rk_march_self_src", "pa_rk_march_vel"):
        strict = name in ("pa_rk_march", "pa_rk_march_src")
        msg = three if strict else two
        add(name, ARG, "order 0", order=0)
        add(name, ARG, "order 4", order=4)
        add(name, ARG, "order 4", order=4, b="a")                      # the order before the buffers
        add(name, ARG, "order 4", order=4, kind=BADKIND)               # ... and before the kind
        add(name, ARG, "bad div kind", b="a", kind=BADKIND)            # the kind before the buffers
        add(name, ARG, msg, b="a")
        add(name, ARG, msg, c="a")
        add(name, ARG, msg, c="b")
        add(name, ARG, msg, nsteps=-1)
        add(name, ARG, msg, final=None)
        add(name, ARG, msg, c=None)
        add(name, ARG, msg, order=3, c=None)
        add(name, ARG, msg, order=1, b="a")
        if strict:
            add(name, ARG, msg, order=1, c=None)
            add(name, ARG, msg, order=1, c="b")
        else:
            add(name, 0, None, order=1, c=None)
            add(name, 0, None, order=1, c="b")                         # w2 is not looked at
    for name in ("pa_rk_march_src", "pa_rk_march_self_src", "pa_rk_march_vel"):
        add(name, ARG, "source field", src=("field", "a"))
        add(name, ARG, "source field", src=("field", "b"))
        add(name, ARG, "source field", src=("field", "c"))
        add(name, ARG, two if name != "pa_rk_march_src" else three, b="a", src=("field", "a"))
    add("pa_rk_march_src", ARG, "source field", uf="x", src=("field", "x"))
    add("pa_rk_march_src", ARG, "source field", order=1, src=("field", "c"))   # three buffers at every order
    add("pa_rk_march_self_src", 0, None, order=1, src=("field", "c"))          # order 1: w2 is no buffer of the call
    add("pa_rk_march_vel", 0, None, order=1, src=("field", "c"))
    add("pa_rk_march_vel", 0, None, order=1, vel=("field", "c"))
    add("pa_rk_march_vel", ARG, "velocity field", vel=("field", "c"))
    # the momentum march
    name, mmsg = "pa_momentum_march", "BC values and nsteps"
    add(name, ARG, "order 0", order=0)
    add(name, ARG, "order 4", order=4)
    add(name, ARG, "order 4", order=4, B="AB")
    add(name, ARG, "order 4", order=4, ncomp=2)
    add(name, ARG, "one component per mesh axis", ncomp=2)
    add(name, ARG, "one component per mesh axis", ncomp=2, kind=COMPAT)
    add(name, ARG, "literal upwind", kind=COMPAT)
    add(name, ARG, "bad div kind", kind=BADKIND)
    add(name, ARG, "bad div kind", kind=BADKIND, nsteps=-1)
    add(name, ARG, mmsg, nsteps=-1)
    add(name, ARG, mmsg, final=None)
    add(name, ARG, mmsg, bcv=None)
    add(name, ARG, mmsg, Cc=None)
    add(name, ARG, mmsg, order=3, Cc=None)
    add(name, ARG, mmsg, nsteps=-1, B="AB")                            # the count before the overlap
    add(name, 0, None, order=1, Cc=None)
    add(name, 0, None, order=1, Cc="AB")                               # w2 is not looked at
    add(name, ARG, "must not overlap", B="AB")
    add(name, ARG, "must not overlap", Cc="AB")
    add(name, ARG, "must not overlap", B="A")
    add(name, ARG, "must not overlap", B="AB", frozen="off")           # the overlap before the frozen velocity
    add(name, ARG, "has == 0", frozen="off")
    add(name, ARG, "frozen velocity field", frozen=("field", "B"))
    add(name, ARG, "has == 0", frozen="off", srcs=("field", "A"))      # the frozen velocity before the sources
    add(name, ARG, "source field must not overlap", srcs=("field", "Cc"))
    add(name, 0, None, order=1, srcs=("field", "Cc"))
    add(name, 0, None, frozen=("field", "X"), srcs=("field", "X"))     # (no test between the velocity and the sources)
    return out


@pytest.mark.parametrize("name,over,rc,word", _cases())
def test_refusals(name, over, rc, word):
    e = _env([6, 6, 8])
    got, msg = e.call(name, **over)
    assert got == rc, (got, msg)
    if word is not None:
        assert word in msg, msg


def test_momentum_needs_one_component_per_axis():
    e = _env([6, 8])
    got, msg = e.call("pa_momentum_march", ncomp=3)
    assert got == ARG and "one component per mesh axis" in msg, (got, msg)
    got, msg = e.call("pa_momentum_march", ncomp=3, order=4)
    assert got == ARG and "order 4" in msg, (got, msg)
    got, msg = e.call("pa_momentum_march", ncomp=2)
    assert got == 0, (got, msg)


@pytest.mark.parametrize("nsteps", [0, 1, 2])
@pytest.mark.parametrize("name", ["pa_rk_march_src", "pa_rk_march_self_src", "pa_rk_march_vel"])
def test_order_one_is_the_ping_pong_of_two_buffers(name, nsteps):
    e = _env([6, 6, 8])
    start = e.t["a"].clone()
    # nsteps calls of the single-step entry
    ref = [start.clone(), torch.empty_like(start)]
    for s in range(nsteps):
        e.t["x"], e.t["y"] = ref[s & 1], ref[(s + 1) & 1]
        if name == "pa_rk_march_vel":
            got, msg = e.call("pa_euler_step_vel", a="x", b="y", src=0.3)
        elif name == "pa_rk_march_self_src":
            got, msg = e.call("pa_euler_step_src", a="x", b="y", u=0.0, uf="x", src=0.3)
        else:
            got, msg = e.call("pa_euler_step_src", a="x", b="y", src=0.3)
        assert got == 0, msg
    # the march
    e.t["x"], e.t["y"], e.t["z"] = start.clone(), torch.full_like(start, -3.0), torch.full_like(start, 7.25)
    got, msg = e.call(name, a="x", b="y", c="z", order=1, nsteps=nsteps, src=0.3)
    assert got == 0, msg
    torch.cuda.synchronize()
    assert e.final.value == (nsteps & 1)
    assert torch.equal(e.t["z"], torch.full_like(start, 7.25))
    res = e.t["x"] if e.final.value == 0 else e.t["y"]
    assert torch.equal(res.view(torch.int64), ref[nsteps & 1].view(torch.int64))
