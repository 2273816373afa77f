// articulation.hip -- the per-env articulated-body step that replaces PhysX's
// gym.simulate (reference: isaacgymenvs/tasks/base/vec_task.py:332-335; model
// and drive set-up tasks/gogoro_new.py:196-294, cfg/task/Gogoro.yaml:9-31).
//
// The step kernel (step_par.h) is specialised per compiled model
// (generated/Model_*.inc, model/codegen.py): 8 lanes per env work through a
// list schedule of the joint tree with the env's articulated state resident in
// LDS.  This file holds the per-env composite cache (compose_kernel), the
// contact-row layout and the dispatch.
//
// Per substep (h = dt / substeps), mirroring oracle/physics_ref.c:
//   1. kinematics + velocities + bias forces (gravity, damping, applied wrench)
//   2. articulated-body inertias with implicit PD drive / limit terms folded
//      into the joint-space diagonal D (h*kd + h^2*kp), effort saturation
//   3. accelerations -> free velocities (semi-implicit Euler, world-fixed root velocity)
//   4. ground contact: static row set per model (normals per shape point,
//      patch friction t1/t2 + torsion), Delassus matrix from impulse
//      responses through the same articulated inertias, projected
//      Gauss-Seidel, one impulse application
//   5. velocity limits, integration of joint positions and the floating base.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "generated/models.inc"
#include "articulation_kernels.h"
#include "launch.h"

namespace tg {

// the compiled-in models' dispatch: this unit's, then the humanoid unit's
// (articulation_tree.hip); TG_OTHER_UNIT: compiled into neither
template <class P>
static int compiled_launch(uint64_t hash, const StepArgs &a, const typename P::Args &pa, hipStream_t stream,
                           hipEvent_t ev_begin, hipEvent_t ev_end) {
    const int rc = unit_launch<P>(hash, a, pa, stream, ev_begin, ev_end);
    return rc == TG_OTHER_UNIT ? tree_launch<P>(hash, a, pa, stream, ev_begin, ev_end) : rc;
}

int launch_step(uint64_t hash, const StepArgs &a, const StepPost &post, hipStream_t stream, hipEvent_t ev_begin,
                hipEvent_t ev_end) {
    int rc = 1;
    // (the force sensor export is declined, 1, by a model without contact
    // rows: it has nothing to read and takes the other exports' kernel)
    if (post.fs && !post.fused())
        rc = compiled_launch<NoPostFS>(hash, a, {post.cf, post.df, post.fs, post.fr}, stream, ev_begin, ev_end);
    if (rc != 1) return rc != TG_OTHER_UNIT ? rc : TG_ERR_MODEL;
    if (post.walk) rc = compiled_launch<WalkPost>(hash, a, *post.walk, stream, ev_begin, ev_end);
    else if (post.gogoro) rc = compiled_launch<GogoroPost>(hash, a, *post.gogoro, stream, ev_begin, ev_end);
    else if (post.paper) rc = compiled_launch<PaperPost>(hash, a, *post.paper, stream, ev_begin, ev_end);
    else if (post.df) rc = compiled_launch<NoPostDF>(hash, a, {post.cf, post.df}, stream, ev_begin, ev_end);
    else if (post.cf) rc = compiled_launch<NoPostCF>(hash, a, {post.cf}, stream, ev_begin, ev_end);
    else rc = compiled_launch<NoPost>(hash, a, {}, stream, ev_begin, ev_end);
    if (rc != TG_OTHER_UNIT) return rc;
    // the run-time (hipRTC) models have the plain step only: no fused epilogue
    // (the caller falls back), no export
    if (post.fused()) return jit_has(hash) ? 1 : TG_ERR_MODEL;
    if (post.cf || post.df || post.fs) return TG_ERR_MODEL;
    return jit_launch_step(hash, a, stream, ev_begin, ev_end);
}

#ifdef TG_DUMP_ENV
// developer build only: select the env whose contact solve the step kernels
// dump (first-substep or the given substep), in BOTH units -- the scooters and
// the known-answer models run in this unit, the humanoid trees in
// articulation_tree.hip -- and read back whichever unit's kernel fired (its
// buffer's word 0 holds the row count; scripts/dev/contact_dump.py)
int tree_dump_arm(int e, int substep);
int tree_dump_read(float *out, int n);
extern "C" int tg_debug_dump_env(int e, int substep) {
    static float zero[4096];
    if (hipMemcpyToSymbol(HIP_SYMBOL(tg_dump_buf), zero, sizeof zero) != hipSuccess) return -2;
    if (hipMemcpyToSymbol(HIP_SYMBOL(tg_dump_sub), &substep, sizeof(int)) != hipSuccess) return -2;
    if (hipMemcpyToSymbol(HIP_SYMBOL(tg_dump_env), &e, sizeof(int)) != hipSuccess) return -2;
    return tree_dump_arm(e, substep);
}
extern "C" int tg_debug_dump_read(float *out, int n) {
    if (n > 4096) n = 4096;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(tg_dump_buf), (size_t)n * 4) != hipSuccess) return -2;
    if (n > 0 && out[0] != 0.f) return 0;          // this unit's kernel dumped
    return tree_dump_read(out, n);              // else the humanoid unit's (or nothing: zeros)
}
#endif

#ifdef TG_SECTION_PROF
// developer builds: the section counters, summed over both units' step kernels
int tree_cprof_read(unsigned long long *out, int n);
int tree_prof_read(unsigned long long *out, int n);
extern "C" int tg_cprof_read(unsigned long long *out, int n) {
    unsigned long long a[8] = {}, b[8] = {};
    if (hipMemcpyFromSymbol(a, HIP_SYMBOL(tg_cprof_acc), sizeof a) != hipSuccess || tree_cprof_read(b, 8)) return -1;
    for (int k = 0; k < n && k < 8; ++k) out[k] = a[k] + b[k];
    return 0;
}
extern "C" int tg_prof_read(unsigned long long *out, int n) {
    unsigned long long a[24] = {}, b[24] = {};
    if (hipMemcpyFromSymbol(a, HIP_SYMBOL(tg_prof_acc), sizeof a) != hipSuccess || tree_prof_read(b, 24)) return -1;
    for (int k = 0; k < n && k < 24; ++k) out[k] = a[k] + b[k];
    return 0;
}
#endif

int compiled_hashes(uint64_t *out, int cap) {
    int n = 0;
#define TG_HASH(MODEL) if (n < cap) out[n] = MODEL::hash; ++n;
    TG_FOR_EACH_MODEL(TG_HASH)
#undef TG_HASH
    return n;
}

// f(M{}) for the compiled-in model M with this hash; false: there is none
template <class F> static bool with_model(uint64_t hash, F &&f) {
#define TG_WITH_MODEL(MODEL) if (hash == MODEL::hash) return f(MODEL{}), true;
    TG_FOR_EACH_MODEL(TG_WITH_MODEL)
#undef TG_WITH_MODEL
    return false;
}

ModelInfo model_info(uint64_t hash) {
    ModelInfo i;
    with_model(hash, [&](auto m) { i = {m.KC, m.NTL, m.EPB, m.FUSED}; });
    return i;
}

template <class... P, class... A>
static int run(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t stream, const A &...args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
    return hipGetLastError() == hipSuccess ? 0 : TG_ERR_HIP;
}

// the on-demand kernels (the list in tg_kernels.h): OnDemand<K, M>::kernel is kernel K's instantiation for model M
template <int K, class M> struct OnDemand;
#define TG_OD_KERNEL(ID, KERNEL) \
    template <class M> struct OnDemand<OD_##ID, M> { static constexpr auto kernel = &KERNEL<M>; };
TG_FOR_EACH_ON_DEMAND(TG_OD_KERNEL)
#undef TG_OD_KERNEL
// (any compiled-in model: a kernel's parameter list does not depend on the model)
template <class M, class...> using FirstOf = M;
#define TG_MODEL_COMMA(MODEL) MODEL,
using AnyModel = FirstOf<TG_FOR_EACH_MODEL(TG_MODEL_COMMA) void>;
#undef TG_MODEL_COMMA
template <class T> struct AsIs { using type = T; };   // (keeps a parameter out of template argument deduction)

// Launches kernel K with the arguments p: a compiled-in model's instantiation, else the run-time model's (jit.cpp)
// with the same grid, block and arguments.  P... are the kernel's own parameter types, so the array of pointers that
// hipModuleLaunchKernel reads has the kernel's count, order and types by construction, and a by-value struct is
// copied once, into p.
template <int K, class... P>
static int on_demand_as(void (*)(P...), uint64_t hash, unsigned grid, unsigned block, hipStream_t stream,
                        typename AsIs<P>::type... p) {
    int rc = 0;
    if (with_model(hash, [&](auto m) {
            constexpr void (*kernel)(P...) = OnDemand<K, decltype(m)>::kernel;   // (every model: the same parameters)
            rc = run(kernel, dim3(grid), dim3(block), stream, p...);
        }))
        return rc;
    void *args[] = {(void *)&p...};
    return jit_launch(hash, K, grid, block, stream, args);
}
// a call's arguments a, converted to the parameter types of kernel K: a wrong count or type does not compile
template <int K, class... A>
static int on_demand(uint64_t hash, unsigned grid, unsigned block, hipStream_t stream, const A &...a) {
    return on_demand_as<K>(OnDemand<K, AnyModel>::kernel, hash, grid, block, stream, a...);
}

int launch_body_states(uint64_t hash, const float *root, const float *dof, int n, float *out, hipStream_t stream) {
    return on_demand<OD_BODY>(hash, n, 64, stream, root, dof, n, out);
}

int launch_jacobians(uint64_t hash, const float *root, const float *dof, int n, float *out, hipStream_t stream) {
    return on_demand<OD_JAC>(hash, n, JAC_THREADS, stream, root, dof, n, out);
}

int launch_mass_matrices(uint64_t hash, const float *root, const float *dof, const float *mass_scale,
                         const float *props, int n, float *out, hipStream_t stream) {
    return on_demand<OD_MASS>(hash, n, 64, stream, root, dof, mass_scale, props, n, out);
}

int launch_ik_dls(uint64_t hash, const float *root, const float *dof, int n, const IkChains &ch, int K,
                  const float *goal_pos, const float *goal_quat, float lambda2, float *dq, float *err,
                  float *pos_targets, hipStream_t stream) {
    return on_demand<OD_IK>(hash, n, 64, stream, root, dof, n, ch, K, goal_pos, goal_quat, lambda2, dq, err,
                            pos_targets);
}

int launch_osc(uint64_t hash, const float *root, const float *dof, const float *mass_scale, const float *props, int n,
               const IkChains &ch, int K, const float *goal_pos, const float *goal_quat, const float *q_rest,
               const OscGains &gains, float *tau, float *err, float *efforts, hipStream_t stream) {
    return on_demand<OD_OSC>(hash, n, 64, stream, root, dof, mass_scale, props, n, ch, K, goal_pos, goal_quat, q_rest,
                             gains, tau, err, efforts);
}

int launch_inverse_dynamics(uint64_t hash, const float *root, const float *dof, const float *mass_scale,
                            const float *props, int n, const IdArgs &ia, const float *accel, float *tau,
                            float *efforts, hipStream_t stream) {
    return on_demand<OD_ID>(hash, n, 64, stream, root, dof, mass_scale, props, n, ia, accel, tau, efforts);
}

int launch_contact_inverse_dynamics(uint64_t hash, const float *root, const float *dof, const float *mass_scale,
                                    const float *props, int n, const IdArgs &ia, const CidArgs &ca, const float *share,
                                    const float *accel, float *tau, float *wrench, float *efforts,
                                    hipStream_t stream) {
    return on_demand<OD_CID>(hash, n, 64, stream, root, dof, mass_scale, props, n, ia, ca, share, accel, tau, wrench,
                             efforts);
}

int launch_centroidal(uint64_t hash, const float *root, const float *dof, const float *mass_scale, int n, float *state,
                      float *matrix, float *bias, hipStream_t stream) {
    return on_demand<OD_CENTROIDAL>(hash, n, 64, stream, root, dof, mass_scale, n, state, matrix, bias);
}

int launch_height_scan(uint64_t hash, const float *root, const float *dof, const float *points, int n,
                       const ScanArgs &sa, float *heights, float *normals, hipStream_t stream) {
    return on_demand<OD_SCAN>(hash, n, 64, stream, root, dof, points, n, sa, heights, normals);
}

int launch_imu(uint64_t hash, const float *root, const float *dof, int n, const ImuArgs &ia, const float *bias,
               const int64_t *reset, float *history, float *out, hipStream_t stream) {
    return on_demand<OD_IMU>(hash, n, 64, stream, root, dof, n, ia, bias, reset, history, out);
}

int launch_ray_cast(uint64_t hash, const float *root, const float *dof, const float *rays, int n, const RayArgs &ra,
                    float *dist, float *normals, hipStream_t stream) {
    return on_demand<OD_RAY>(hash, (unsigned)n * (unsigned)ray_chunks(ra), 64, stream, root, dof, rays, n, ra, dist,
                             normals);
}

int launch_proximity(uint64_t hash, const float *root, const float *dof, int n, const ProxArgs &pa, float *dist,
                     float *witness, float *summary, hipStream_t stream) {
    return on_demand<OD_PROX>(hash, n, 64, stream, root, dof, n, pa, dist, witness, summary);
}

int launch_contact_qp(uint64_t hash, const float *root, const float *dof, const float *mass_scale, const float *props,
                      int n, const IdArgs &ia, const QpArgs &qa, const float *normals, const float *friction,
                      const float *share, const float *accel, float *tau, float *wrench, float *forces, float *info,
                      float *efforts, hipStream_t stream) {
    return on_demand<OD_QP>(hash, n, 64, stream, root, dof, mass_scale, props, n, ia, qa, normals, friction, share,
                            accel, tau, wrench, forces, info, efforts);
}

int launch_rb_forces(uint64_t hash, const float *root, const float *dof, const float *comp, int n,
                     const float *mass_scale, const float *forces, const float *torques, int space, float *out,
                     const float *props, hipStream_t stream) {
    return on_demand<OD_RBF>(hash, (n + COMPOSE_WPB - 1) / COMPOSE_WPB, 64 * COMPOSE_WPB, stream, root, dof, comp, n,
                             mass_scale, forces, torques, space, out, props);
}

// the full compose of launch_compose (launch.h), shared-cache check included:
// the flag a later step kernel reads describes the blocks this launch wrote
int launch_compose_only(uint64_t hash, const StepArgs &a, hipStream_t stream) {
    int rc = 0;
    return with_model(hash, [&](auto m) {
        rc = run(compose_kernel<decltype(m)>, dim3((a.N + COMPOSE_WPB - 1) / COMPOSE_WPB), dim3(64 * COMPOSE_WPB),
                 stream, a);
        if (rc == 0 && a.cuni) {
            if (hipMemsetD32Async(a.cuni, 1, 1, stream) != hipSuccess) rc = TG_ERR_HIP;
            else rc = run(uniform_check_kernel<decltype(m)>, dim3(a.N), dim3(64), stream, a);
        }
    }) ? rc : TG_ERR_MODEL;
}

}  // namespace tg

