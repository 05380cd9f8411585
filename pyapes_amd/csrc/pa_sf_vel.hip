// pa_sf_vel.hip -- the VEL instantiations of k_sf (pa_sf_kernel.h): the upwind explicit Euler step and the fused Runge-Kutta
// stage in a velocity field, one advection speed per mesh axis (pa_*_vel).  Three scalar speeds (VEL 1) or three speed fields
// read at the cell (VEL 2), two rows per wave, with and without a source term.  Everything else with a velocity -- central,
// QUICK, 1-D / 2-D meshes, odd rows, unaligned operands, a periodic axis 0, a mix of scalar and field components, n1 <= 4 --
// runs the generic k_euler (pa_march.hip): pa_tile3d_euler_vel returns 0 for it.  A target that is itself one of the three speed
// fields (pa_momentum_march, own >= 0) takes the VEL 3 instantiations of pa_sf_vself.hip under the same conditions.
#include "pa_sf_kernel.h"

template <typename T, int VEL, bool STG>
static int launch_sf_vel(pa_ctx* c, Cg3dArgs<T>& A, bool source) {
  return source ? launch_sf<T, 2, 3, PA_OP_DIV_UPWIND, false, false, 0, STG, false, true, VEL>(c, A)
                : launch_sf<T, 2, 3, PA_OP_DIV_UPWIND, false, false, 0, STG, false, false, VEL>(c, A);
}

template <typename T>
int pa_sf_euler_vel(pa_ctx* c, Cg3dArgs<T>& A, bool stage, bool fields, bool source) {
  if (fields) return stage ? launch_sf_vel<T, 2, true>(c, A, source) : launch_sf_vel<T, 2, false>(c, A, source);
  return stage ? launch_sf_vel<T, 1, true>(c, A, source) : launch_sf_vel<T, 1, false>(c, A, source);
}

// vel: indexed by INTERNAL axis (step_t, pa_march.hip).  Blocks launched, 0 when k_sf does not take the launch, < 0: error.
template <typename T>
int pa_tile3d_euler_vel(pa_ctx* c, Vec<T> phi, T* out, int kind, const pa_velocity* vel, double nu, double dt, const T* phi0,
                        double c0, double c1, const pa_source* src, int own) {
  if (kind != PA_OP_DIV_UPWIND || c->ndim != 3) return 0;
  const int nf = (vel->field[0] ? 1 : 0) + (vel->field[1] ? 1 : 0) + (vel->field[2] ? 1 : 0);
  if (nf != 0 && nf != 3) return 0;                  // a mix of scalar and field components
  if (c->G.n1 <= 4) return 0;                        // two rows per wave only
  if (c->bc[0].type == PA_BC_PERIODIC || c->bc[1].type == PA_BC_PERIODIC) return 0;   // a periodic axis 0
  DevEq<T> E;
  pa_build_lap<T>(c, E);
  // (the three speed fields, a stage's phi0 and a source field count for the alignment)
  const int mode = cg3d_mode<T>(c, E, {phi.p, out, phi.glo, phi.ghi, phi0, src ? src->field : nullptr, vel->field[0], vel->field[1],
                                       vel->field[2]});
  if (!mode) return 0;
  Cg3dArgs<T> A;
  memset(&A, 0, sizeof(A));
  fill_common<T>(c, E, A);
  fill_h<T>(c, A);
  A.d = phi; A.out = out; A.p0 = (T)nu; A.p1 = (T)dt; A.kind = kind;
  A.stg_phi0 = phi0; A.stg_c0 = (T)c0; A.stg_c1 = (T)c1;
  if (src) { A.src = (const T*)src->field; A.src_val = (T)src->value; }
  for (int a = 0; a < 3; ++a) { A.vel_f[a] = (const T*)vel->field[a]; A.vel_v[a] = (T)vel->value[a]; }
  A.out_all = pa_bc_on_every_face(c);   // the BC fill that follows the step kernel rewrites every face plane that has a BC (pa_tile3d_euler)
  if (!sf_applies<T, 3>(c, A, mode)) return 0;
  A.vel_own = own;
  const bool vself = own >= 0 && own < 3 && nf == 3 && c->vself && vel->field[own] == (const void*)phi.p;
  const int n = vself ? pa_sf_euler_vself<T>(c, A, phi0 != nullptr, src != nullptr)
                      : pa_sf_euler_vel<T>(c, A, phi0 != nullptr, nf == 3, src != nullptr);
  if (n > 0 && hipGetLastError() != hipSuccess) { pa_set_err(c, "k_sf Euler launch (velocity) failed"); return PA_E_HIP; }
  return n;
}

template int pa_sf_euler_vel<float>(pa_ctx*, Cg3dArgs<float>&, bool, bool, bool);
template int pa_sf_euler_vel<double>(pa_ctx*, Cg3dArgs<double>&, bool, bool, bool);
template int pa_tile3d_euler_vel<float>(pa_ctx*, Vec<float>, float*, int, const pa_velocity*, double, double, const float*, double, double, const pa_source*, int);
template int pa_tile3d_euler_vel<double>(pa_ctx*, Vec<double>, double*, int, const pa_velocity*, double, double, const double*, double, double, const pa_source*, int);
