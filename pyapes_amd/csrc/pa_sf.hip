// pa_sf.hip -- the single-field operations on a tiled mesh: A x (Laplacian, Div, Laplacian + Div), the
// explicit Euler step, the explicit gradient.  The instruction-heavy ones -- everything with a Div term --
// run on k_sf (pa_sf_kernel.h: wave-autonomous marching, no LDS, no barrier) where rows are whole 16-byte
// vectors; the Laplacian alone and the gradient stay on k_cg3d's phases 2 / 7 (pa_cg3d_kernel.h), which move
// their 2 / 4 passes at the speed of a device copy, as does everything k_sf does not take (odd row lengths,
// unaligned operands, tensor coefficient, 2-D meshes).
// pa_tile3d_step is the one entry of a step (step_t, pa_march.hip) into the tiled layer: it fills the arguments, declines what
// no tiled kernel takes, and hands the variant record (sf_variant, pa_sf_kernel.h) to the unit that holds the instantiation.
// This unit holds the plain k_sf instantiations of the three Div schemes, phases 2 and 3; the others -- SELF, SRC, VEL, k_sfq
// -- are units of their own because this one is already the slowest of the parallel build.
#include "pa_sf_kernel.h"

// PHASE 2 (A x) or 3 (Euler step / stage): scalar speed -- for upwind with its sign, US 1 / 2 -- or a speed field read at the cell;
// one, two or four rows per wave; BC on load for the upwind step, two or four rows
template <typename T, int PHASE>
static int launch_sf_any(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  if (V.self || V.src || V.vel) return 0;
  return with_int<PA_OP_DIV_CENTRAL, PA_OP_DIV_UPWIND_COMPAT, PA_OP_DIV_UPWIND>(V.kind, [&](auto kind) {
    return with_bool(V.stg, [&](auto stg) {
      return with_bool(V.hasu, [&](auto hasu) {
        constexpr int KIND = decltype(kind)::value;
        constexpr bool STG = decltype(stg)::value, HASU = decltype(hasu)::value;
        if constexpr (STG && PHASE != 3) {
          return 0;
        } else if constexpr (KIND == PA_OP_DIV_UPWIND && !HASU) {
          return with_int<0, 1, 2>(V.us, [&](auto us) {   // (US 0: the form a build with PA_SF_USIGN 0 launches)
            constexpr int US = decltype(us)::value;
            if constexpr (PHASE == 3) {
              if (V.bcl) return launch_sf_rows<T, 3, KIND, false, true, US, STG, false, false, 0, 2, 4>(c, A, V);
            }
            return V.bcl ? 0 : launch_sf_rows<T, PHASE, KIND, false, false, US, STG, false, false, 0, 1, 2, 4>(c, A, V);
          });
        } else {
          if (V.us) return 0;
          if constexpr (PHASE == 3 && KIND == PA_OP_DIV_UPWIND) {
            if (V.bcl) return launch_sf_rows<T, 3, KIND, true, true, 0, STG, false, false, 0, 2, 4>(c, A, V);
          }
          return V.bcl ? 0 : launch_sf_rows<T, PHASE, KIND, HASU, false, 0, STG, false, false, 0, 1, 2, 4>(c, A, V);
        }
      });
    });
  });
}

template <typename T>
int pa_sf_launch(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) { return launch_sf_any<T, 3>(c, A, V); }

// vel: indexed by INTERNAL axis (step_t, pa_march.hip)
template <typename T>
int pa_tile3d_step(pa_ctx* c, Vec<T> phi, T* out, const StepRequest<T>& rq) {
  const DevGeom& G = c->G;
  const int kind = rq.adv.kind;
  const pa_velocity* vel = rq.adv.vel;
  const pa_source* src = rq.src;
  const T* phi0 = rq.stage.phi0;
  const void* u_field = vel ? nullptr : rq.adv.u_field;
  const bool limited = kind == PA_OP_DIV_MINMOD || kind == PA_OP_DIV_MC;
  const bool reach2 = !vel && (kind == PA_OP_DIV_QUICK || limited);   // k_sfq or nothing
  // the field advects itself: the speed at the cell and at its neighbours are the stencil's own operands (k_sf SELF)
  const bool self = u_field && u_field == (const void*)phi.p;
  const T* nuf = (const T*)rq.nu_field;
  if (nuf) {   // a diffusivity field: k_sfn -- upwind, one scalar speed, no source, two rows per wave, one GPU -- or nothing
    if (vel || u_field || src || rq.bcl || kind != PA_OP_DIV_UPWIND || c->ndim != 3 || G.n1 <= 4 || c->slab || G.n0 != G.g0) return 0;
  }
  if (vel) {   // k_sf VEL or nothing
    if (kind != PA_OP_DIV_UPWIND || c->ndim != 3) return 0;
    const int nf = (vel->field[0] ? 1 : 0) + (vel->field[1] ? 1 : 0) + (vel->field[2] ? 1 : 0);
    if (nf != 0 && nf != 3) return 0;                  // a mix of scalar and field components
    if (G.n1 <= 4) return 0;                           // two rows per wave only
    if (c->bc[0].type == PA_BC_PERIODIC || c->bc[1].type == PA_BC_PERIODIC) return 0;   // a periodic axis 0
  } else if (reach2) {
    if (limited && src) return 0;   // no SRC instantiations of the limited schemes (pa_sft.hip): the generic kernel
    if (!c->sfq || !c->sf || c->slab || c->ndim != 3 || !G.act[0] || G.n0 != G.g0 || G.off0 != 0) return 0;
    if (G.n0 < 5 || G.n1 < 5 || G.n2 < 5) return 0;
    if (G.bct[0] == PA_BC_PERIODIC || G.bct[1] == PA_BC_PERIODIC) return 0;   // the planes beyond the ends are not wrapped
  }
  DevEq<T> E;
  pa_build_lap<T>(c, E);
  // (the speed fields, a stage's phi0 and a source field count for the alignment)
  const void* sfield = src ? src->field : nullptr;
  const int mode = vel ? cg3d_mode<T>(c, E, {phi.p, out, phi.glo, phi.ghi, phi0, sfield, vel->field[0], vel->field[1], vel->field[2]})
                       : cg3d_mode<T>(c, E, {phi.p, out, u_field, phi.glo, phi.ghi, phi0, sfield, nuf});
  if (!mode || (reach2 && mode != 1)) return 0;   // k_sfq: whole 16-byte vectors, aligned operands
  const bool one_speed = !vel && !reach2;   // k_sf, or k_cg3d's Euler phase where k_sf does not apply
  if (one_speed) {
    if (src && kind == PA_OP_DIV_UPWIND_COMPAT) return 0;   // no SRC instantiation of the literal form: generic kernel
    if (kind == PA_OP_DIV_CENTRAL && u_field && !self) return 0;  // needs a foreign u at the neighbours: generic kernel
  }
  Cg3dArgs<T> A;
  memset(&A, 0, sizeof(A));
  fill_common<T>(c, E, A);
  fill_h<T>(c, A);
  A.d = phi; A.out = out; A.p0 = (T)rq.nu; A.p1 = (T)rq.dt; A.kind = kind;
  if (!vel) { A.aux = (const T*)u_field; A.u = (T)rq.adv.u; }
  A.stg_phi0 = phi0; A.stg_c0 = (T)rq.stage.c0; A.stg_c1 = (T)rq.stage.c1;   // phi0 != null: the Runge-Kutta stage (STG instantiations)
  if (src) { A.src = (const T*)src->field; A.src_val = (T)src->value; }   // the SRC instantiations
  if (vel) {
    for (int a = 0; a < 3; ++a) { A.vel_f[a] = (const T*)vel->field[a]; A.vel_v[a] = (T)vel->value[a]; }
    A.vel_own = rq.adv.own;
  }
  // the kernels write the step's value at EVERY node where the BC fill that follows (step_t) rewrites every face plane that has a BC
  A.out_all = pa_bc_on_every_face(c);
  if (nuf) {   // w_a as the generic kernel's launch forms it (step_t): each operation rounded in T
    A.nu_f = nuf;
    for (int a = 0; a < 3; ++a) {
      T w = A.ih[a] * A.ih[a];
      w = (T)0.5 * w;
      A.nu_w[a] = w;
    }
  }
  const bool sf = sf_applies<T, 3>(c, A, mode);
  if (nuf && !sf) return 0;   // k_cg3d's Euler phase knows no diffusivity field: the generic kernel does
  if (!one_speed && !sf) return 0;
  if (src && !sf) return 0;   // k_cg3d's Euler phase takes no source: the generic kernel does
  // central self off k_sf: k_cg3d reads the speed at the cell only.  On a slab the generic kernel takes u's axis-0
  // neighbours from the rank's own planes, k_sf would take the ghost planes: the generic kernel keeps its bits
  if (one_speed && kind == PA_OP_DIV_CENTRAL && self && (!sf || G.n0 != G.g0)) return 0;
  if (one_speed && rq.bcl) {   // BC on load (k_sf only): the fill values of the face interiors are formed from the stencil's own operands
    if (!A.out_all || !sf || kind != PA_OP_DIV_UPWIND) return 0;
    A.bcl_c43 = (T)(4.0 / 3.0);
    A.bcl_c13 = (T)(1.0 / 3.0);
    for (int f = 0; f < 6; ++f) {
      const HostBC& b = c->bc[f];
      if (b.vals || b.type < PA_BC_DIRICHLET || b.type > PA_BC_SYMMETRY) return 0;
      A.bcl_type[f] = b.type;
      if (b.type == PA_BC_DIRICHLET) A.bcl_val[f] = (T)b.value;
      if (b.type == PA_BC_NEUMANN) {   // the additive constant as pa_bc.hip forms it
        T pre = (T)((2.0 / 3.0) * b.value);
        pre = pre * (T)b.dxf;
        pre = pre * ((f & 1) == 0 ? (T)-1 : (T)1);
        A.bcl_val[f] = pre;
      }
    }
  }
  const int n = sf ? sf_launch_variant<T>(c, A, sf_variant<T>(c, A, src != nullptr, self, vel != nullptr))
                   : with_bool(phi0 != nullptr, [&](auto stg) { return launch_any<T, 3, decltype(stg)::value>(c, A, mode); });
  if (n > 0 && hipGetLastError() != hipSuccess) { pa_set_err(c, "tiled Euler step launch failed"); return PA_E_HIP; }
  return n;
}

template <typename T>
int pa_tile3d_aop(pa_ctx* c, const DevEq<T>& E, Vec<T> x, T* y, int interior_only) {
  const int mode = cg3d_mode<T>(c, E, {x.p, y, x.glo, x.ghi}, true, true);
  if (!mode) return 0;
  Cg3dArgs<T> A;
  memset(&A, 0, sizeof(A));
  fill_common<T>(c, E, A);
  A.d = x; A.out = y; A.interior_only = interior_only;
  if (A.lap_off) A.aux = E.t[0].u_f;  // explicit upwind Div with a speed field (null: scalar speed)
  int n = 0;
  // the Laplacian alone stays on k_cg3d: both kernels move it at the speed of a device copy (512^3 fp64
  // 0.416 vs 0.423 ms, fp32 0.192 vs 0.200; a copy: 0.414 / 0.200), as they do the gradient
  if (A.kind != 0 && sf_applies<T, 2>(c, A, mode)) {
    n = launch_sf_any<T, 2>(c, A, sf_variant<T>(c, A));   // Laplacian + Div, or the Div term alone (lap_off)
  } else {
    n = launch_any<T, 2>(c, A, mode);
  }
  if (n > 0 && hipGetLastError() != hipSuccess) { pa_set_err(c, "k_cg3d A x launch failed"); return PA_E_HIP; }
  return n;
}

// explicit gradient, nd components of ncell each (k_grad): geometry / mode check as for a Laplacian
template <typename T>
int pa_tile3d_grad(pa_ctx* c, Vec<T> x, T* y, int nd) {
  DevEq<T> E;
  pa_build_lap<T>(c, E);
  const int mode = cg3d_mode<T>(c, E, {x.p, y, x.glo, x.ghi});
  if (!mode || nd != c->ndim) return 0;
  Cg3dArgs<T> A;
  memset(&A, 0, sizeof(A));
  fill_common<T>(c, E, A);
  A.grd = E.grd;
  A.gnd = nd;
  A.d = x; A.out = y;
  int n = launch_any<T, 7>(c, A, mode);
  if (n > 0 && hipGetLastError() != hipSuccess) { pa_set_err(c, "k_cg3d grad launch failed"); return PA_E_HIP; }
  return n;
}

template int pa_sf_launch<float>(pa_ctx*, Cg3dArgs<float>&, const SfVariant&);
template int pa_sf_launch<double>(pa_ctx*, Cg3dArgs<double>&, const SfVariant&);
template int pa_tile3d_step<float>(pa_ctx*, Vec<float>, float*, const StepRequest<float>&);
template int pa_tile3d_step<double>(pa_ctx*, Vec<double>, double*, const StepRequest<double>&);
template int pa_tile3d_grad<float>(pa_ctx*, Vec<float>, float*, int);
template int pa_tile3d_grad<double>(pa_ctx*, Vec<double>, double*, int);
template int pa_tile3d_aop<float>(pa_ctx*, const DevEq<float>&, Vec<float>, float*, int);
template int pa_tile3d_aop<double>(pa_ctx*, const DevEq<double>&, Vec<double>, double*, int);
