// tgsim_api.cpp -- host side of the C-ABI (include/tgsim.h, include/tg_gogoro.h).
//
// Owns the per-sim device buffers (struct-of-arrays where the kernels want
// coalescing, the reference's AoS row layouts where the Python side expects
// IsaacGym-compatible tensor views), validates every call and reports errors
// through tg_last_error().  All work is stream-ordered on the sim's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/tg_gogoro.h"
#include "../../include/tg_gogoro_paper.h"
#include "../../include/tgsim.h"
#include "tg_kernels.h"

namespace {
thread_local std::string g_err;

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return fail(TG_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_)); \
    } while (0)
}  // namespace

struct tg_sim {
    int device = 0;
    int N = 0, D = 0, G = 0, L = 0, S = 0, KC = 0;
    uint64_t hash = 0;
    tg_sim_params params{};
    hipStream_t stream = nullptr;
    float gravity[3] = {0, 0, -9.81f};
    bool forces_pending = false;
    // apply_rigid_body_force_tensors waiting for the next simulate: reduced to
    // group wrenches by that simulate's compose launch, or by rb_force_kernel
    bool rbf_pending = false;
    const float *rbf_f = nullptr, *rbf_t = nullptr;
    int rbf_space = 0;
    // some env may be dirty (its composite cache stale): set by every call that
    // can mark envs dirty or change what compose reads (creation, state
    // binding, tg_refresh -- the contract for writes through the zero-copy
    // views --, property / mass-scale setters, the Gogoro and paper task
    // kernels, whose resets rewrite properties), cleared by a compose launch.
    // While false, a simulate without a compose prologue skips the compose
    // launch (one launch less per step; ThormangWalk's envs never go dirty)
    bool dirty_possible = true;
    // reset lists of the fused Gogoro epilogue (compose_list_kernel): two
    // slots of N ids + counts; the epilogue appends to slot list_cur, the next
    // compose reads the other one and zeroes list_cur's count; list_pending:
    // the last step kernel had that epilogue (its resets await their compose)
    int *clist = nullptr, *ccount = nullptr;
    int list_cur = 0;
    bool list_pending = false;
    // device buffers
    float *root = nullptr, *dof = nullptr, *pos_tgt = nullptr, *vel_tgt = nullptr, *act = nullptr;
    float *props = nullptr, *force = nullptr, *mass_scale = nullptr, *shape_mu = nullptr, *comp = nullptr;
    float *zero_link3 = nullptr;   // [N*L*3] zeros (torque-only rigid-body force calls), lazily allocated
    // net contact force tensor [N,L,3] (tg_set_net_contact_force_tensor), caller-owned; null: off
    float *cf = nullptr;
    // DOF force tensor [N,D] (tg_set_dof_force_tensor), caller-owned; null: off
    float *df = nullptr;
    // force sensor tensor [N,S,6] (tg_set_force_sensor_tensor), caller-owned, with its frames; null: off
    float *fs = nullptr;
    tg::FsFrames fs_frames{};
    float *env_origin = nullptr;
    uint8_t *dirty = nullptr;
    int *err = nullptr;   // sticky state-error flag set by kernels (tg_sync reports it)
    // shared-cache flag (StepArgs::cuni) for compiled-in models whose task
    // kernels never edit composites / properties in place (not FUSED 2|4)
    int *cuni = nullptr;
    bool uni_ok = false;
    // terrain heightfield (tg_set_heightfield)
    float *hf = nullptr;
    int hf_rows = 0, hf_cols = 0;
    float hf_hs = 0.f, hf_vs = 0.f, hf_ox = 0.f, hf_oy = 0.f, hf_mu = 0.f;
    float hf_zcap = 0.f;   // no vertex is higher than this (formed on the host; tg_ray_cast skips the air above it)
    std::vector<void *> allocs;
    // kernel timing (tg_set_kernel_timing): event pairs recorded, not yet read
    bool walk_unfused = false;   // tg_walk_step: separate post-physics launch (TG_WALK_UNFUSED=1)
    bool post_unfused = false;   // tg_gogoro_step: separate post-physics launch (TG_POST_UNFUSED=1)
    bool always_compose = false; // never skip the compose launch (TG_ALWAYS_COMPOSE=1)
    bool pre_in_compose = false; // tg_walk_step: pre-physics in the compose launch, not the step kernel (TG_PRE_IN_COMPOSE=1)
    bool no_inplace = false;     // tg_gogoro_step: reset envs re-composed, not updated in place (TG_SEAT_RECOMPOSE=1)
    bool paper_finish_launch = false;   // tg_paper_step: term 7 summed by the finish launch (TG_PAPER_FINISH=1)
    bool paper_rb_launch = false;       // tg_paper_step: rb_forces reduced by rb_force_kernel (TG_PAPER_RB_LAUNCH=1)
    bool paper_two_launch = false;      // tg_paper_step: step kernel + post launch, never one launch (TG_PAPER_TWO_LAUNCH=1)
    // tg_paper_step in one launch (PaperPost): the term-7 arrival counter and
    // the total it reaches after the last launch; the device's CU count (the
    // grid must be resident at once)
    unsigned *t7cnt = nullptr;
    unsigned t7_total = 0;
    int num_cus = 0;
    int timing = 0;          // period (0: off; < 0: windows of -timing launches)
    int64_t timing_count = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending, ev_free;
    std::vector<int> ev_launches;   // step-kernel launches each pending pair brackets
    // windowed timing (tg_set_kernel_timing with a negative period): one event
    // pair around -timing consecutive step-kernel launches, dropped when any
    // other launch of the library falls inside it (win_dirty)
    std::pair<hipEvent_t, hipEvent_t> win{nullptr, nullptr};
    int win_n = 0;
    bool win_dirty = false;
    // tg_paper_step reduced its rb_forces (rbf_f) to the next simulate's group
    // wrenches already, from the state it left; any later call that can change
    // that state (every other launching entry point, tg_refresh, tg_bind_state)
    // turns them back into a pending tensor, reduced at the next simulate
    bool rbf_prereduced = false;
    double timed_ms = 0.0;
    int64_t timed_launches = 0;
    // launch statistics (tg_debug_launch_stats): plain host counters, kept by
    // simulate_args -- [0] full compose launches, [1] list compose launches,
    // [2] simulates that skipped the compose, [3] launch_rb_forces launches,
    // [4] pending force tensors reduced inside a compose, [5] fused launches
    // declined (rc 1)
    int64_t stats[6] = {0, 0, 0, 0, 0, 0};

    template <class T> int alloc(T **p, size_t count) {
        void *q = nullptr;
        if (count == 0) count = 1;
        hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e != hipSuccess) return fail(TG_ERR_HIP, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
        e = hipMemset(q, 0, count * sizeof(T));
        if (e != hipSuccess) return fail(TG_ERR_HIP, "hipMemset: %s", hipGetErrorString(e));
        allocs.push_back(q);
        *p = (T *)q;
        return 0;
    }
    ~tg_sim() {
        for (void *p : allocs) (void)hipFree(p);
        if (hf) (void)hipFree(hf);
        for (auto *v : {&ev_pending, &ev_free})
            for (auto &e : *v) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        if (win.first) { (void)hipEventDestroy(win.first); (void)hipEventDestroy(win.second); }
    }
};

namespace {
// a launch other than the step kernel: an open timing window no longer
// brackets step kernels only
inline void win_touch(tg_sim *s) {
    if (s->win.first) s->win_dirty = true;
    if (s->rbf_prereduced) {
        s->rbf_pending = true;
        s->rbf_prereduced = false;
    }
}

int check_sim(tg_sim *s) { return s ? 0 : fail(TG_ERR_ARG, "null tg_sim"); }
int check_ids(tg_sim *s, const int32_t *ids, int32_t n) {
    if (n < 0 || n > s->N) return fail(TG_ERR_ARG, "index count %d out of range [0, %d]", n, s->N);
    if (n > 0 && !ids) return fail(TG_ERR_ARG, "null index pointer with n=%d", n);
    return 0;
}
// the sim's heightfield of this moment (null: no terrain) into any kernel argument struct that has the members
// ground_at (ground.h) reads: StepArgs, ScanArgs, RayArgs
template <class A> void heightfield_args(const tg_sim *s, A &a) {
    a.hf = s->hf_rows > 0 ? s->hf : nullptr;
    a.hf_rows = s->hf_rows;
    a.hf_cols = s->hf_cols;
    a.hf_hs = s->hf_hs;
    a.hf_vs = s->hf_vs;
    a.hf_ox = s->hf_ox;
    a.hf_oy = s->hf_oy;
}
// The link frames of a sensor call (tg_height_scan, tg_imu, tg_ray_cast), in the two phases of their checks.  L < 0,
// before the sim is looked at: no negative link and no offset that is not finite, and the frames are copied to dst.
// Otherwise, after it: every link within the model's L.  what: the word of the messages, "frame" or "sensor"
int check_link_frames(const char *fn, const char *what, const tg_contact_frame *f, int n, int L,
                      tg_contact_frame *dst = nullptr) {
    for (int k = 0; k < n; ++k) {
        if (L >= 0) {
            if (f[k].link >= L)
                return fail(TG_ERR_ARG, "%s: %s %d: link %d outside [0, %d)", fn, what, k, f[k].link, L);
            continue;
        }
        if (f[k].link < 0) return fail(TG_ERR_ARG, "%s: %s %d: link %d is negative", fn, what, k, f[k].link);
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(f[k].offset[i]))
                return fail(TG_ERR_ARG, "%s: %s %d: offset[%d] is not finite", fn, what, k, i);
        dst[k] = f[k];
    }
    return 0;
}
tg::StepArgs step_args(tg_sim *s) {
    tg::StepArgs a{};
    const tg_sim_params &p = s->params;
    a.N = s->N;
    a.D = s->D;
    a.h = p.substeps > 0 ? p.dt / (float)p.substeps : 0.f;   // (0 substeps: tg_set_sim_params replay mode)
    a.substeps = p.substeps;
    a.gx = s->gravity[0]; a.gy = s->gravity[1]; a.gz = s->gravity[2];
    a.lin_damp = p.linear_damping;
    a.ang_damp = p.angular_damping;
    a.max_depen = p.max_depenetration_velocity;
    a.rest = p.rest_offset;
    a.margin = p.contact_margin;
    a.coff = p.contact_offset;
    a.ground_mu = p.ground_friction;
    a.baumgarte = p.baumgarte;
    a.lim_k = p.limit_stiffness;
    a.lim_c = p.limit_damping;
    a.iters = p.contact_iterations;
    a.viters = p.velocity_iterations;
    a.fix_base = p.fix_base;
    a.tgs = p.solver_type == 1 && p.contact_iterations > 0;
    a.root = s->root;
    a.dof = s->dof;
    a.pos_tgt = s->pos_tgt;
    a.vel_tgt = s->vel_tgt;
    a.act = s->act;
    a.props = s->props;
    a.force = s->forces_pending ? s->force : nullptr;
    a.shape_mu = s->shape_mu;
    a.mass_scale = s->mass_scale;
    a.comp = s->comp;
    a.dirty = s->dirty;
    a.err = s->err;
    a.cuni = s->uni_ok ? s->cuni : nullptr;
    heightfield_args(s, a);
    a.hf_mu = s->hf_mu;
    return a;
}
}  // namespace

extern "C" {

const char *tg_last_error(void) { return g_err.c_str(); }

uint64_t tg_compiled_model_hashes(uint64_t *out, int32_t cap) { return (uint64_t)tg::compiled_hashes(out, cap); }

int tg_model_jit(uint64_t model_hash, const char *struct_name, const char *model_source, const char *include_dir,
                 const char *cache_dir) {
    if (!struct_name || !model_source) return fail(TG_ERR_ARG, "tg_model_jit: null argument");
    if (tg::model_info(model_hash).kc >= 0 && !tg::jit_has(model_hash)) return TG_OK;   // compiled in
    std::string err;
    if (int rc = tg::jit_compile(model_hash, struct_name, model_source, include_dir, cache_dir, err))
        return fail(rc, "tg_model_jit(0x%016llx): %s", (unsigned long long)model_hash, err.c_str());
    return TG_OK;
}

int tg_sim_create(const tg_model_desc *m, const tg_sim_params *params, int32_t num_envs, int32_t device,
                  tg_sim **out) {
    if (!m || !params || !out) return fail(TG_ERR_ARG, "tg_sim_create: null argument");
    *out = nullptr;
    if (num_envs <= 0) return fail(TG_ERR_ARG, "num_envs must be positive (got %d)", num_envs);
    if (params->substeps <= 0 || !(params->dt > 0.f)) return fail(TG_ERR_ARG, "dt and substeps must be positive");
    if (params->contact_iterations < 0 || params->velocity_iterations < 0)
        return fail(TG_ERR_ARG, "contact / velocity iterations must be >= 0");
    if (params->solver_type != 0 && params->solver_type != 1)
        return fail(TG_ERR_ARG, "solver_type must be 0 (PGS) or 1 (TGS), got %d", params->solver_type);
    int kc = tg::model_info(m->model_hash).kc;
    if (kc < 0) kc = tg::jit_kc(m->model_hash);   // a run-time model
    if (kc < 0)
        return fail(TG_ERR_MODEL,
                    "model hash 0x%016llx has no specialisation in libtgsim.so: compiled-in models are listed by "
                    "tg_compiled_model_hashes; any other model must first be compiled with tg_model_jit",
                    (unsigned long long)m->model_hash);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(TG_ERR_ARG, "device %d not present (%d visible)", device, ndev);
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<tg_sim> owner(new tg_sim());   // released to the caller on success only
    tg_sim *s = owner.get();
    if (const char *u = getenv("TG_WALK_UNFUSED")) s->walk_unfused = u[0] == '1';
    if (const char *u = getenv("TG_POST_UNFUSED")) s->post_unfused = u[0] == '1';
    if (const char *u = getenv("TG_ALWAYS_COMPOSE")) s->always_compose = u[0] == '1';
    if (const char *u = getenv("TG_PRE_IN_COMPOSE")) s->pre_in_compose = u[0] == '1';
    if (const char *u = getenv("TG_SEAT_RECOMPOSE")) s->no_inplace = u[0] == '1';
    if (const char *u = getenv("TG_PAPER_FINISH")) s->paper_finish_launch = u[0] == '1';
    if (const char *u = getenv("TG_PAPER_RB_LAUNCH")) s->paper_rb_launch = u[0] == '1';
    if (const char *u = getenv("TG_PAPER_TWO_LAUNCH")) s->paper_two_launch = u[0] == '1';
    // (TG_NO_SHARED_CACHE=1: every env reads its own block, the A/B control)
    const char *nsc = getenv("TG_NO_SHARED_CACHE");
    s->uni_ok = !(nsc && nsc[0] == '1') && (tg::model_info(m->model_hash).fused & 6) == 0 && !tg::jit_has(m->model_hash);
    s->device = device;
    s->N = num_envs;
    s->D = m->num_dofs;
    s->G = m->num_groups;
    s->L = m->num_links;
    s->S = m->num_shapes;
    s->KC = kc;
    s->hash = m->model_hash;
    s->params = *params;
    memcpy(s->gravity, params->gravity, sizeof s->gravity);
    const size_t N = num_envs;
    int rc = 0;
    rc |= s->alloc(&s->root, N * 13);
    rc |= s->alloc(&s->dof, N * s->D * 2);
    rc |= s->alloc(&s->pos_tgt, N * s->D);
    rc |= s->alloc(&s->vel_tgt, N * s->D);
    rc |= s->alloc(&s->act, N * s->D);
    rc |= s->alloc(&s->props, (size_t)TG_NUM_PROPS * N * s->D);
    rc |= s->alloc(&s->force, N * s->G * 6);
    rc |= s->alloc(&s->mass_scale, N * s->L);
    rc |= s->alloc(&s->shape_mu, N * (s->S > 0 ? s->S : 1));
    rc |= s->alloc(&s->comp, (size_t)kc * N);
    rc |= s->alloc(&s->env_origin, N * 3);
    rc |= s->alloc(&s->dirty, N);
    rc |= s->alloc(&s->err, 1);
    rc |= s->alloc(&s->cuni, 1);   // 0: not uniform until a compose checked it
    rc |= s->alloc(&s->clist, 2 * N);
    rc |= s->alloc(&s->ccount, 2);
    if (rc) return TG_ERR_HIP;   // g_err holds the failing allocation; owner frees the rest
    // host-side initial values: identity root pose at the env origin grid,
    // unit mass scale, per-shape friction from the model, defaults for props
    std::vector<float> h_root(N * 13, 0.f), h_org(N * 3, 0.f), h_ms(N * s->L, 1.f);
    std::vector<float> h_mu(N * (s->S > 0 ? s->S : 1), 1.f);
    std::vector<uint8_t> h_dirty(N, 1);
    const int per_row = params->envs_per_row > 0 ? params->envs_per_row : 1;
    for (size_t e = 0; e < N; ++e) {
        h_org[3 * e + 0] = 2.f * params->env_spacing * (float)(e % per_row);
        h_org[3 * e + 1] = 2.f * params->env_spacing * (float)(e / per_row);
        h_root[13 * e + 0] = h_org[3 * e + 0];
        h_root[13 * e + 1] = h_org[3 * e + 1];
        h_root[13 * e + 6] = 1.f;
        for (int k = 0; k < s->S; ++k) h_mu[e * s->S + k] = m->shape_friction[k];
    }
    std::vector<float> h_props((size_t)TG_NUM_PROPS * N * s->D, 0.f);
    for (size_t i = 0; i < N * s->D; ++i) {
        h_props[(size_t)TG_PROP_LOWER * N * s->D + i] = -3.4e38f;
        h_props[(size_t)TG_PROP_UPPER * N * s->D + i] = 3.4e38f;
    }
    HIPCHK(hipMemcpy(s->root, h_root.data(), h_root.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->env_origin, h_org.data(), h_org.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->mass_scale, h_ms.data(), h_ms.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->shape_mu, h_mu.data(), h_mu.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->dirty, h_dirty.data(), N, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(s->ccount, 0, 2 * sizeof(int)));
    HIPCHK(hipMemcpy(s->props, h_props.data(), h_props.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    *out = owner.release();
    return TG_OK;
}

int tg_sim_destroy(tg_sim *s) {
    if (!s) return TG_OK;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    delete s;
    return TG_OK;
}

int tg_set_stream(tg_sim *s, void *stream) {
    if (int rc = check_sim(s)) return rc;
    s->stream = (hipStream_t)stream;
    return TG_OK;
}

int tg_state_ptrs(tg_sim *s, tg_state_view *v) {
    if (int rc = check_sim(s)) return rc;
    if (!v) return fail(TG_ERR_ARG, "null view");
    v->root_state = s->root;
    v->dof_state = s->dof;
    v->dof_pos_target = s->pos_tgt;
    v->dof_vel_target = s->vel_tgt;
    v->dof_actuation = s->act;
    v->dof_props = s->props;
    v->body_force = s->force;
    v->env_origin = s->env_origin;
    v->env_dirty = s->dirty;
    v->num_envs = s->N;
    v->num_dofs = s->D;
    v->num_groups = s->G;
    v->num_links = s->L;
    return TG_OK;
}

int tg_refresh(tg_sim *s) {
    if (int rc = check_sim(s)) return rc;
    s->dirty_possible = true;   // writes through the zero-copy views (env_dirty, dof_props) take effect
    win_touch(s);
    return TG_OK;
}

int tg_bind_state(tg_sim *s, const tg_state_view *v) {
    if (int rc = check_sim(s)) return rc;
    s->dirty_possible = true;
    win_touch(s);
    if (!v) return fail(TG_ERR_ARG, "null view");
    const size_t N = s->N, D = s->D;
    struct B {
        void *src;
        void **dst;
        size_t bytes;
    } binds[] = {
        {v->root_state, (void **)&s->root, N * 13 * 4},
        {v->dof_state, (void **)&s->dof, N * D * 2 * 4},
        {v->dof_pos_target, (void **)&s->pos_tgt, N * D * 4},
        {v->dof_vel_target, (void **)&s->vel_tgt, N * D * 4},
        {v->dof_actuation, (void **)&s->act, N * D * 4},
        {v->dof_props, (void **)&s->props, (size_t)TG_NUM_PROPS * N * D * 4},
        {v->body_force, (void **)&s->force, N * s->G * 6 * 4},
        {v->env_origin, (void **)&s->env_origin, N * 3 * 4},
        {v->env_dirty, (void **)&s->dirty, N},
    };
    for (auto &b : binds) {
        if (!b.src || b.src == *b.dst) continue;
        HIPCHK(hipMemcpyAsync(b.src, *b.dst, b.bytes, hipMemcpyDeviceToDevice, s->stream));
        *b.dst = b.src;
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    return TG_OK;
}

static int copy_full(tg_sim *s, float *dst, const float *src, size_t count) {
    if (!src) return fail(TG_ERR_ARG, "null source tensor");
    if (src == dst) return TG_OK;
    if (s->win.first) s->win_dirty = true;   // (a copy inside a timing window)
    HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
    return TG_OK;
}

int tg_set_dof_position_targets(tg_sim *s, const float *pos) {
    if (int rc = check_sim(s)) return rc;
    return copy_full(s, s->pos_tgt, pos, (size_t)s->N * s->D);
}
int tg_set_dof_velocity_targets(tg_sim *s, const float *vel) {
    if (int rc = check_sim(s)) return rc;
    return copy_full(s, s->vel_tgt, vel, (size_t)s->N * s->D);
}
int tg_set_dof_actuation_forces(tg_sim *s, const float *eff) {
    if (int rc = check_sim(s)) return rc;
    return copy_full(s, s->act, eff, (size_t)s->N * s->D);
}

int tg_set_actor_root_state_indexed(tg_sim *s, const float *root, const int32_t *ids, int32_t n) {
    if (int rc = check_sim(s)) return rc;
    if (int rc = check_ids(s, ids, n)) return rc;
    if (!root) return fail(TG_ERR_ARG, "null root state");
    if (root == s->root) return TG_OK;
    win_touch(s);
    if (int rc = tg::launch_scatter_rows(s->root, root, ids, n, 13, s->stream)) return fail(rc, "scatter failed");
    return TG_OK;
}

int tg_set_dof_state_indexed(tg_sim *s, const float *dof, const int32_t *ids, int32_t n) {
    if (int rc = check_sim(s)) return rc;
    if (int rc = check_ids(s, ids, n)) return rc;
    if (!dof) return fail(TG_ERR_ARG, "null dof state");
    if (dof == s->dof) return TG_OK;
    win_touch(s);
    if (int rc = tg::launch_scatter_rows(s->dof, dof, ids, n, 2 * s->D, s->stream)) return fail(rc, "scatter failed");
    return TG_OK;
}

int tg_set_dof_properties_indexed(tg_sim *s, int32_t field, const float *vals, const int32_t *ids, int32_t n) {
    if (int rc = check_sim(s)) return rc;
    s->dirty_possible = true;
    if (int rc = check_ids(s, ids, n)) return rc;
    if (field < 0 || field >= TG_NUM_PROPS) return fail(TG_ERR_ARG, "unknown dof property field %d", field);
    if (!vals) return fail(TG_ERR_ARG, "null property values");
    float *dst = s->props + (size_t)field * s->N * s->D;
    win_touch(s);
    if (vals != dst) {   // (writes through the zero-copy props view need no copy)
        if (int rc = tg::launch_scatter_field(dst, vals, ids, n, s->D, s->stream)) return fail(rc, "scatter failed");
    }
    if (int rc = tg::launch_mark_dirty(s->dirty, ids, n, s->stream)) return fail(rc, "mark dirty failed");
    return TG_OK;
}

int tg_set_body_mass_scale_indexed(tg_sim *s, const float *scale, const int32_t *ids, int32_t n) {
    if (int rc = check_sim(s)) return rc;
    s->dirty_possible = true;
    if (int rc = check_ids(s, ids, n)) return rc;
    if (!scale) return fail(TG_ERR_ARG, "null mass scale");
    win_touch(s);
    if (int rc = tg::launch_scatter_rows(s->mass_scale, scale, ids, n, s->L, s->stream)) return fail(rc, "scatter failed");
    win_touch(s);
    if (int rc = tg::launch_mark_dirty(s->dirty, ids, n, s->stream)) return fail(rc, "mark dirty failed");
    return TG_OK;
}

int tg_set_shape_friction_indexed(tg_sim *s, const float *mu, const int32_t *ids, int32_t n) {
    if (int rc = check_sim(s)) return rc;
    if (int rc = check_ids(s, ids, n)) return rc;
    if (!mu) return fail(TG_ERR_ARG, "null friction");
    if (s->S == 0) return TG_OK;
    win_touch(s);
    if (int rc = tg::launch_scatter_rows(s->shape_mu, mu, ids, n, s->S, s->stream)) return fail(rc, "scatter failed");
    return TG_OK;
}

int tg_set_gravity(tg_sim *s, const float *g3) {
    if (int rc = check_sim(s)) return rc;
    if (!g3) return fail(TG_ERR_ARG, "null gravity");
    memcpy(s->gravity, g3, sizeof s->gravity);
    return TG_OK;
}

int tg_apply_body_forces(tg_sim *s, const float *wrench) {
    if (int rc = check_sim(s)) return rc;
    if (!wrench) return fail(TG_ERR_ARG, "null wrench tensor");
    if (int rc = copy_full(s, s->force, wrench, (size_t)s->N * s->G * 6)) return rc;
    s->forces_pending = true;
    s->rbf_pending = false;   // the group wrenches given here replace a pending per-link tensor
    s->rbf_prereduced = false;
    return TG_OK;
}

int tg_set_heightfield(tg_sim *s, const float *heights, int32_t rows, int32_t cols, float horizontal_scale,
                       float vertical_scale, float origin_x, float origin_y, float friction) {
    if (int rc = check_sim(s)) return rc;
    if (rows == 0) {
        s->hf_rows = s->hf_cols = 0;
        return TG_OK;
    }
    if (!heights || rows < 2 || cols < 2) return fail(TG_ERR_ARG, "heightfield needs >= 2 x 2 samples");
    if (!(horizontal_scale > 0.f)) return fail(TG_ERR_ARG, "heightfield horizontal_scale must be > 0");
    HIPCHK(hipStreamSynchronize(s->stream));
    if (s->hf) {
        HIPCHK(hipFree(s->hf));
        s->hf = nullptr;
    }
    const size_t bytes = (size_t)rows * cols * sizeof(float);
    HIPCHK(hipMalloc(&s->hf, bytes));
    HIPCHK(hipMemcpy(s->hf, heights, bytes, hipMemcpyHostToDevice));
    s->hf_rows = rows;
    s->hf_cols = cols;
    s->hf_hs = horizontal_scale;
    s->hf_vs = vertical_scale;
    s->hf_ox = origin_x;
    s->hf_oy = origin_y;
    s->hf_mu = friction;
    // the highest vertex, with a margin far above fp32 rounding so that a ray clipped to z <= hf_zcap loses no hit;
    // FLT_MAX (no clipping) when a sample is not finite
    float zmax = -FLT_MAX;
    for (size_t k = 0; k < (size_t)rows * cols; ++k) {
        const float z = vertical_scale * heights[k];
        if (!std::isfinite(z)) {
            zmax = FLT_MAX;
            break;
        }
        zmax = std::max(zmax, z);
    }
    s->hf_zcap = zmax < FLT_MAX ? zmax + 1e-4f * std::max(1.f, std::fabs(zmax)) : FLT_MAX;
    return TG_OK;
}

// compose (+ optional prologue in a) and the step kernel of one simulate call;
// with a fused epilogue in post, the step kernel carrying that post-physics
// (returns 1, nothing launched, when the model has no such instantiation)
// makes the sim's device current for the launches of one call (per-device
// kernel attributes, tg_set_stream's stream), restoring the caller's device
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

static int simulate_args(tg_sim *s, const tg::StepArgs &a_in, tg::StepPost post = {}) {
    // the net contact force, DOF force and force sensor exports have no
    // fused-epilogue variant: the task steps take their general path
    // (simulates, then the post-physics launch)
    if ((s->cf || s->df || s->fs) && post.fused()) {
        s->stats[5]++;
        return 1;
    }
    post.cf = s->cf;
    post.df = s->df;
    post.fs = s->fs;
    post.fr = s->fs_frames;
    DeviceGuard dg(s->device);
    tg::StepArgs a = a_in;
    // the compose launch: every dirty env (host-side changes possible), the
    // last fused epilogue's reset list, the task prologue alone, or none
    const bool walk_prologue = a.pm_actions && !a.pm_in_step;
    const bool gogoro_prologue = a.gp.actions && !a.gp_in_step;
    // (a pending per-link force tensor with listed envs: the full compose, which
    // reduces it after composing them)
    const bool paper_prologue = a.pp.actions && !a.pp_in_step;   // (one wavefront per env: the full compose launch)
    const bool full = s->dirty_possible || s->always_compose || walk_prologue || paper_prologue ||
                      (s->rbf_pending && s->list_pending);
    a.skip_compose = !full && !s->list_pending && !gogoro_prologue;
    a.compose_list = !full && !a.skip_compose;
    a.cnext = s->ccount + s->list_cur;
    if (a.compose_list && s->list_pending) {
        const int prev = 1 - s->list_cur;
        a.clist = s->clist + (size_t)prev * s->N;
        a.ccount = s->ccount + prev;
    }
    bool rb_launch = false, rb_in_compose = false;
    if (s->rbf_pending) {   // the pending per-link forces: in the full compose launch, else on their own
        if (!a.skip_compose && !a.compose_list) {
            // reduced by the compose launch below: still pending until that
            // launch went through (a fused launcher may decline the call,
            // rc 1, and the caller's fallback simulate must reduce them then)
            rb_in_compose = true;
            a.rbf_forces = s->rbf_f;
            a.rbf_torques = s->rbf_t;
            a.rbf_space = s->rbf_space;
            a.rbf_out = s->force;
        } else {
            rb_launch = true;
            if (int rc = tg::launch_rb_forces(s->hash, s->root, s->dof, s->comp, (int)s->N, s->mass_scale, s->rbf_f,
                                              s->rbf_t, s->rbf_space, s->force, s->props, s->stream))
                return fail(rc, "rigid-body force launch failed");
            s->stats[3]++;
            s->rbf_pending = false;   // s->force holds the reduced wrenches now
        }
    }
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    const bool timed = s->timing > 0 && s->timing_count % s->timing == 0;
    // windowed timing: this call launches a compose / rigid-body force kernel
    // too (other), or only the step kernel
    const bool windowed = s->timing < 0, other = !a.skip_compose || rb_launch;
    if (windowed && s->win.first && other) s->win_dirty = true;
    if (windowed && !s->win.first && !other) {
        if (!s->ev_free.empty()) {
            s->win = s->ev_free.back();
            s->ev_free.pop_back();
        } else {
            HIPCHK(hipEventCreate(&s->win.first));
            HIPCHK(hipEventCreate(&s->win.second));
        }
        s->win_n = 0;
        s->win_dirty = false;
        HIPCHK(hipEventRecord(s->win.first, s->stream));
    }
    if (timed) {
        if (!s->ev_free.empty()) {
            ev = s->ev_free.back();
            s->ev_free.pop_back();
        } else {
            HIPCHK(hipEventCreate(&ev.first));
            HIPCHK(hipEventCreate(&ev.second));
        }
    }
    const int rc = tg::launch_step(s->hash, a, post, s->stream, ev.first, ev.second);
    // the pair joins the pending list only once both events were recorded by a
    // launch that went through; otherwise it goes back to the free list
    if (rc != 0) {
        if (ev.first) s->ev_free.push_back(ev);
        if (s->win.first) {   // the open window is dropped
            s->ev_free.push_back(s->win);
            s->win = {nullptr, nullptr};
        }
        if (rc == 1) {   // not launched (no such instantiation): caller falls back
            s->stats[5]++;
            return 1;
        }
        return fail(rc, "step launch failed: %s", hipGetErrorString(hipGetLastError()));
    }
    s->stats[a.skip_compose ? 2 : (a.compose_list ? 1 : 0)]++;
    if (rb_in_compose) {
        s->rbf_pending = false;
        s->stats[4]++;
    }
    if (s->timing > 0) s->timing_count++;
    if (ev.first) {
        s->ev_pending.push_back(ev);
        s->ev_launches.push_back(1);
    }
    if (windowed && s->win.first && ++s->win_n == -s->timing) {   // the window closes
        if (!s->win_dirty) {
            HIPCHK(hipEventRecord(s->win.second, s->stream));
            s->ev_pending.push_back(s->win);
            s->ev_launches.push_back(s->win_n);
        } else {
            s->ev_free.push_back(s->win);
        }
        s->win = {nullptr, nullptr};
    }
    s->forces_pending = false;   // apply_rigid_body_force_tensors acts for one simulate call
    s->rbf_prereduced = false;
    if (!a.skip_compose) {   // every dirty env, or every listed one, is composed now
        if (!a.compose_list) s->dirty_possible = false;
        s->list_pending = false;
    }
    if (post.gogoro && !post.gogoro->tl_inplace) {   // the Gogoro epilogue's resets rewrite properties
        if (post.gogoro->reset_list) {                // ... and are listed for the next compose
            s->list_pending = true;
            s->list_cur = 1 - s->list_cur;
        } else {
            s->dirty_possible = true;
        }
    }
    return TG_OK;
}

int tg_get_sim_params(tg_sim *s, tg_sim_params *out) {
    if (int rc = check_sim(s)) return rc;
    if (!out) return fail(TG_ERR_ARG, "tg_get_sim_params: null output");
    *out = s->params;
    memcpy(out->gravity, s->gravity, sizeof s->gravity);
    return TG_OK;
}

int tg_set_sim_params(tg_sim *s, const tg_sim_params *p) {
    if (int rc = check_sim(s)) return rc;
    if (!p) return fail(TG_ERR_ARG, "tg_set_sim_params: null argument");
    if (p->substeps < 0 || !(p->dt > 0.f)) return fail(TG_ERR_ARG, "dt must be positive and substeps >= 0");
    if (p->contact_iterations < 0 || p->velocity_iterations < 0)
        return fail(TG_ERR_ARG, "contact / velocity iterations must be >= 0");
    if (p->solver_type != 0 && p->solver_type != 1)
        return fail(TG_ERR_ARG, "solver_type must be 0 (PGS) or 1 (TGS), got %d", p->solver_type);
    const float spacing = s->params.env_spacing;
    const int32_t per_row = s->params.envs_per_row, fix_base = s->params.fix_base;
    s->params = *p;
    s->params.env_spacing = spacing;   // the env grid is fixed at creation,
    s->params.envs_per_row = per_row;
    s->params.fix_base = fix_base;     // and so is the asset option fix_base_link
    memcpy(s->gravity, p->gravity, sizeof s->gravity);
    return TG_OK;
}

int tg_simulate(tg_sim *s) {
    if (int rc = check_sim(s)) return rc;
    return simulate_args(s, step_args(s));
}

int tg_apply_rigid_body_force_tensors(tg_sim *s, const float *forces, const float *torques, int32_t space) {
    if (int rc = check_sim(s)) return rc;
    if (!forces && !torques) return fail(TG_ERR_ARG, "apply_rigid_body_force_tensors: no force or torque tensor");
    if (space != TG_ENV_SPACE && space != TG_LOCAL_SPACE) return fail(TG_ERR_ARG, "space must be TG_ENV_SPACE or TG_LOCAL_SPACE");
    DeviceGuard dg(s->device);
    const float *f = forces;
    if (!f) {   // torques only: a zero force tensor
        if (!s->zero_link3) {
            if (int rc = s->alloc(&s->zero_link3, (size_t)s->N * s->L * 3)) return fail(rc, "allocation failed");
            HIPCHK(hipMemsetAsync(s->zero_link3, 0, (size_t)s->N * s->L * 3 * 4, s->stream));
        }
        f = s->zero_link3;
    }
    // reduced when the next simulate runs (PhysX applies the forces during
    // simulate, at the state it starts from): inside its compose launch if it
    // has one, else by rb_force_kernel just before the step
    s->rbf_f = f;
    s->rbf_t = torques;
    s->rbf_space = space;
    s->rbf_pending = true;
    s->rbf_prereduced = false;
    s->forces_pending = true;
    return TG_OK;
}

int tg_rigid_body_states(tg_sim *s, float *out) {
    if (int rc = check_sim(s)) return rc;
    if (!out) return fail(TG_ERR_ARG, "tg_rigid_body_states: null output");
    win_touch(s);
    if (int rc = tg::launch_body_states(s->hash, s->root, s->dof, (int)s->N, out, s->stream))
        return fail(rc, "rigid-body state launch failed");
    return TG_OK;
}

int tg_jacobians(tg_sim *s, float *out) {
    if (int rc = check_sim(s)) return rc;
    if (!out) return fail(TG_ERR_ARG, "tg_jacobians: null output");
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_jacobians(s->hash, s->root, s->dof, (int)s->N, out, s->stream))
        return fail(rc, "Jacobian launch failed");
    return TG_OK;
}

int tg_mass_matrices(tg_sim *s, float *out) {
    if (int rc = check_sim(s)) return rc;
    if (!out) return fail(TG_ERR_ARG, "tg_mass_matrices: null output");
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_mass_matrices(s->hash, s->root, s->dof, s->mass_scale, s->props, (int)s->N, out,
                                          s->stream))
        return fail(rc, "mass-matrix launch failed");
    return TG_OK;
}

// the per-chain checks tg_ik_dls and tg_osc share (num_chains already in 1..TG_IK_MAX_CHAINS); fn: the call's
// name for the message
static int check_chains(const tg_sim *s, const char *fn, const tg_ik_chain *chains, int32_t num_chains,
                        tg::IkChains &ch) {
    for (int k = 0; k < num_chains; ++k) {
        const tg_ik_chain &c = chains[k];
        if (c.link < 0 || c.link >= s->L)
            return fail(TG_ERR_ARG, "%s: chain %d: link %d outside [0, %d)", fn, k, c.link, s->L);
        if (c.num_dofs < 1 || c.num_dofs > TG_IK_MAX_DOFS)
            return fail(TG_ERR_ARG, "%s: chain %d: num_dofs %d outside 1..%d", fn, k, c.num_dofs, TG_IK_MAX_DOFS);
        for (int i = 0; i < c.num_dofs; ++i) {
            if (c.dofs[i] < 0 || c.dofs[i] >= s->D)
                return fail(TG_ERR_ARG, "%s: chain %d: DOF %d outside [0, %d)", fn, k, c.dofs[i], s->D);
            for (int j = 0; j < i; ++j)
                if (c.dofs[j] == c.dofs[i])
                    return fail(TG_ERR_ARG, "%s: chain %d: DOF %d appears twice", fn, k, c.dofs[i]);
        }
        ch.c[k] = c;
        for (int i = c.num_dofs; i < TG_IK_MAX_DOFS; ++i) ch.c[k].dofs[i] = 0;   // ignored entries: nothing stale reaches the kernel
    }
    return TG_OK;
}

int tg_ik_dls(tg_sim *s, const tg_ik_chain *chains, int32_t num_chains, const float *goal_pos,
              const float *goal_quat, float damping, float *dq, float *err, float *pos_targets) {
    if (int rc = check_sim(s)) return rc;
    if (!chains || !goal_pos) return fail(TG_ERR_ARG, "tg_ik_dls: null %s", !chains ? "chains" : "goal_pos");
    if (num_chains < 1 || num_chains > TG_IK_MAX_CHAINS)
        return fail(TG_ERR_ARG, "tg_ik_dls: num_chains %d outside 1..%d", num_chains, TG_IK_MAX_CHAINS);
    if (!(damping > 0.f) || !std::isfinite(damping))
        return fail(TG_ERR_ARG, "tg_ik_dls: damping %g is not a finite number > 0", (double)damping);
    if (!dq && !err && !pos_targets) return fail(TG_ERR_ARG, "tg_ik_dls: dq, err and pos_targets are all null");
    tg::IkChains ch{};
    if (int rc = check_chains(s, "tg_ik_dls", chains, num_chains, ch)) return rc;
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_ik_dls(s->hash, s->root, s->dof, (int)s->N, ch, num_chains, goal_pos, goal_quat,
                                   damping * damping, dq, err, pos_targets, s->stream))
        return fail(rc, "tg_ik_dls: launch failed");
    return TG_OK;
}

int tg_osc(tg_sim *s, const tg_ik_chain *chains, int32_t num_chains, const float *goal_pos, const float *goal_quat,
           const float *q_rest, const tg_osc_gains *gains, float *tau, float *err, float *efforts) {
    if (int rc = check_sim(s)) return rc;
    if (!chains || !goal_pos || !gains)
        return fail(TG_ERR_ARG, "tg_osc: null %s", !chains ? "chains" : (!goal_pos ? "goal_pos" : "gains"));
    if (num_chains < 1 || num_chains > TG_IK_MAX_CHAINS)
        return fail(TG_ERR_ARG, "tg_osc: num_chains %d outside 1..%d", num_chains, TG_IK_MAX_CHAINS);
    const tg_osc_gains g = *gains;
    if (!(g.damping > 0.f) || !std::isfinite(g.damping))
        return fail(TG_ERR_ARG, "tg_osc: damping %g is not a finite number > 0", (double)g.damping);
    const struct { const char *name; float v; } gs[] = {{"kp", g.kp}, {"kd", g.kd}, {"kp_null", g.kp_null},
                                                       {"kd_null", g.kd_null}};
    for (const auto &x : gs)
        if (!(x.v >= 0.f) || !std::isfinite(x.v))
            return fail(TG_ERR_ARG, "tg_osc: %s %g is not a finite number >= 0", x.name, (double)x.v);
    if (!tau && !err && !efforts) return fail(TG_ERR_ARG, "tg_osc: tau, err and efforts are all null");
    tg::IkChains ch{};
    if (int rc = check_chains(s, "tg_osc", chains, num_chains, ch)) return rc;
    DeviceGuard dg(s->device);
    win_touch(s);
    const tg::OscGains kg{g.kp, g.kd, g.kp_null, g.kd_null, g.damping * g.damping};
    if (int rc = tg::launch_osc(s->hash, s->root, s->dof, s->mass_scale, s->props, (int)s->N, ch, num_chains, goal_pos,
                                goal_quat, q_rest, kg, tau, err, efforts, s->stream))
        return fail(rc, "tg_osc: launch failed");
    return TG_OK;
}

// the checks tg_inverse_dynamics and tg_contact_inverse_dynamics share, and the IdArgs they fill; fn: the call's
// name for the message
static int check_id_terms(const char *fn, int32_t terms, const float *accel) {
    if (terms < 0 || terms > (TG_ID_GRAVITY | TG_ID_VELOCITY))
        return fail(TG_ERR_ARG, "%s: terms %d outside 0..%d", fn, terms, TG_ID_GRAVITY | TG_ID_VELOCITY);
    if (terms == 0 && !accel) return fail(TG_ERR_ARG, "%s: no terms and no accel", fn);
    return TG_OK;
}
static int check_id_dofs(const tg_sim *s, const char *fn, int32_t terms, const float *efforts, const int32_t *dofs,
                         int32_t num_dofs, int32_t accumulate, tg::IdArgs &ia) {
    if (num_dofs < 0 || num_dofs > s->D) return fail(TG_ERR_ARG, "%s: num_dofs %d outside 0..%d", fn, num_dofs, s->D);
    if (num_dofs > 0 && !dofs) return fail(TG_ERR_ARG, "%s: null dofs with num_dofs %d", fn, num_dofs);
    constexpr int MASK_BITS = 32 * tg::TG_ID_MASK_WORDS;
    if (efforts && s->D > MASK_BITS)
        return fail(TG_ERR_ARG, "%s: efforts of a model with %d DOFs, more than %d", fn, s->D, MASK_BITS);
    for (int i = 0; i < num_dofs; ++i) {
        const int d = dofs[i];
        if (d < 0 || d >= s->D) return fail(TG_ERR_ARG, "%s: DOF %d outside [0, %d)", fn, d, s->D);
        for (int j = 0; j < i; ++j)
            if (dofs[j] == d) return fail(TG_ERR_ARG, "%s: DOF %d appears twice", fn, d);
        if (d < MASK_BITS) ia.mask[d >> 5] |= 1u << (d & 31);   // (beyond it only without efforts: nothing reads the mask)
    }
    if (num_dofs == 0)   // every DOF
        for (int d = 0; d < s->D && d < MASK_BITS; ++d) ia.mask[d >> 5] |= 1u << (d & 31);
    memcpy(ia.g, s->gravity, sizeof ia.g);
    ia.terms = terms;
    ia.accumulate = accumulate != 0;
    return TG_OK;
}

int tg_inverse_dynamics(tg_sim *s, int32_t terms, const float *accel, float *tau, float *efforts,
                        const int32_t *dofs, int32_t num_dofs, int32_t accumulate) {
    if (!s) return fail(TG_ERR_ARG, "tg_inverse_dynamics: null tg_sim");
    const char *fn = "tg_inverse_dynamics";
    if (int rc = check_id_terms(fn, terms, accel)) return rc;
    if (!tau && !efforts) return fail(TG_ERR_ARG, "%s: tau and efforts are both null", fn);
    tg::IdArgs ia{};
    if (int rc = check_id_dofs(s, fn, terms, efforts, dofs, num_dofs, accumulate, ia)) return rc;
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_inverse_dynamics(s->hash, s->root, s->dof, s->mass_scale, s->props, (int)s->N, ia, accel, tau,
                                             efforts, s->stream))
        return fail(rc, "tg_inverse_dynamics: launch failed");
    return TG_OK;
}

int tg_contact_inverse_dynamics(tg_sim *s, const tg_contact_frame *contacts, int32_t num_contacts, const float *share,
                                float moment_arm, int32_t terms, const float *accel, float *tau, float *wrench,
                                float *efforts, const int32_t *dofs, int32_t num_dofs, int32_t accumulate) {
    const char *fn = "tg_contact_inverse_dynamics";
    if (!s) return fail(TG_ERR_ARG, "%s: null tg_sim", fn);
    if (!contacts) return fail(TG_ERR_ARG, "%s: null contacts", fn);
    if (num_contacts < 1 || num_contacts > TG_CID_MAX_CONTACTS)
        return fail(TG_ERR_ARG, "%s: num_contacts %d outside 1..%d", fn, num_contacts, TG_CID_MAX_CONTACTS);
    tg::CidArgs ca{};
    for (int k = 0; k < num_contacts; ++k) {
        const int l = contacts[k].link;
        if (l < 0 || l >= s->L) return fail(TG_ERR_ARG, "%s: contact %d: link %d outside [0, %d)", fn, k, l, s->L);
        for (int j = 0; j < k; ++j)
            if (contacts[j].link == l) return fail(TG_ERR_ARG, "%s: link %d appears twice", fn, l);
        ca.c[k] = contacts[k];
    }
    if (!(moment_arm > 0.f) || !std::isfinite(moment_arm))
        return fail(TG_ERR_ARG, "%s: moment_arm %g is not a finite number > 0", fn, (double)moment_arm);
    if (int rc = check_id_terms(fn, terms, accel)) return rc;
    if (!tau && !wrench && !efforts) return fail(TG_ERR_ARG, "%s: tau, wrench and efforts are all null", fn);
    tg::IdArgs ia{};
    if (int rc = check_id_dofs(s, fn, terms, efforts, dofs, num_dofs, accumulate, ia)) return rc;
    ca.K = num_contacts;
    ca.arm2 = moment_arm * moment_arm;
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_contact_inverse_dynamics(s->hash, s->root, s->dof, s->mass_scale, s->props, (int)s->N, ia,
                                                     ca, share, accel, tau, wrench, efforts, s->stream))
        return fail(rc, "%s: launch failed", fn);
    return TG_OK;
}

int tg_contact_qp(tg_sim *s, const tg_contact_frame *contacts, int32_t num_contacts, const float *extents,
                  const float *normals, const float *friction, float mu, const float *share, float moment_arm,
                  float reg, float rho, float relax, int32_t iters, int32_t terms, const float *accel, float *tau,
                  float *wrench, float *forces, float *info, float *efforts, const int32_t *dofs, int32_t num_dofs,
                  int32_t accumulate) {
    const char *fn = "tg_contact_qp";
    if (!s) return fail(TG_ERR_ARG, "%s: null tg_sim", fn);
    if (!contacts) return fail(TG_ERR_ARG, "%s: null contacts", fn);
    if (!extents) return fail(TG_ERR_ARG, "%s: null extents", fn);
    if (num_contacts < 1 || num_contacts > TG_CID_MAX_CONTACTS)
        return fail(TG_ERR_ARG, "%s: num_contacts %d outside 1..%d", fn, num_contacts, TG_CID_MAX_CONTACTS);
    tg::QpArgs qa{};
    for (int k = 0; k < num_contacts; ++k) {
        const int l = contacts[k].link;
        if (l < 0 || l >= s->L) return fail(TG_ERR_ARG, "%s: contact %d: link %d outside [0, %d)", fn, k, l, s->L);
        for (int j = 0; j < k; ++j)
            if (contacts[j].link == l) return fail(TG_ERR_ARG, "%s: link %d appears twice", fn, l);
        qa.c[k] = contacts[k];
    }
    for (int k = 0; k < num_contacts; ++k)
        for (int i = 0; i < 2; ++i) {
            const float h = extents[2 * k + i];
            if (!(h >= 0.f) || !std::isfinite(h))
                return fail(TG_ERR_ARG, "%s: contact %d: extent[%d] %g is not a finite number >= 0", fn, k, i, (double)h);
            qa.ext[k][i] = h;
        }
    if (!(mu >= 0.f) || !std::isfinite(mu))
        return fail(TG_ERR_ARG, "%s: mu %g is not a finite number >= 0", fn, (double)mu);
    if (!(moment_arm > 0.f) || !std::isfinite(moment_arm))
        return fail(TG_ERR_ARG, "%s: moment_arm %g is not a finite number > 0", fn, (double)moment_arm);
    if (!(reg > 0.f) || !std::isfinite(reg))
        return fail(TG_ERR_ARG, "%s: reg %g is not a finite number > 0", fn, (double)reg);
    if (!(rho > 0.f) || !std::isfinite(rho))
        return fail(TG_ERR_ARG, "%s: rho %g is not a finite number > 0", fn, (double)rho);
    if (!(relax > 0.f && relax < 2.f)) return fail(TG_ERR_ARG, "%s: relax %g outside (0, 2)", fn, (double)relax);
    if (iters < 1 || iters > TG_QP_MAX_ITERS)
        return fail(TG_ERR_ARG, "%s: iters %d outside 1..%d", fn, iters, TG_QP_MAX_ITERS);
    if (int rc = check_id_terms(fn, terms, accel)) return rc;
    if (!tau && !wrench && !forces && !info && !efforts)
        return fail(TG_ERR_ARG, "%s: tau, wrench, forces, info and efforts are all null", fn);
    tg::IdArgs ia{};
    if (int rc = check_id_dofs(s, fn, terms, efforts, dofs, num_dofs, accumulate, ia)) return rc;
    qa.K = num_contacts;
    qa.arm2 = moment_arm * moment_arm;
    qa.mu = mu;
    qa.reg = reg;
    qa.rho = rho;
    qa.relax = relax;
    qa.iters = iters;
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_contact_qp(s->hash, s->root, s->dof, s->mass_scale, s->props, (int)s->N, ia, qa, normals,
                                       friction, share, accel, tau, wrench, forces, info, efforts, s->stream))
        return fail(rc, "%s: launch failed", fn);
    return TG_OK;
}

int tg_centroidal(tg_sim *s, float *state, float *matrix, float *bias) {
    if (!s) return fail(TG_ERR_ARG, "tg_centroidal: null tg_sim");
    if (!state && !matrix && !bias) return fail(TG_ERR_ARG, "tg_centroidal: state, matrix and bias are all null");
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_centroidal(s->hash, s->root, s->dof, s->mass_scale, (int)s->N, state, matrix, bias,
                                       s->stream))
        return fail(rc, "tg_centroidal: launch failed");
    return TG_OK;
}

int tg_height_scan(tg_sim *s, const tg_contact_frame *frames, int32_t num_frames, const float *points,
                   int32_t num_points, const tg_scan_params *params, float *heights, float *normals) {
    const char *fn = "tg_height_scan";
    // everything that can be judged without the sim first, then the sim, then the links against its model
    if (!frames) return fail(TG_ERR_ARG, "%s: null frames", fn);
    if (!points) return fail(TG_ERR_ARG, "%s: null points", fn);
    if (!params) return fail(TG_ERR_ARG, "%s: null params", fn);
    if (num_frames < 1 || num_frames > TG_SCAN_MAX_FRAMES)
        return fail(TG_ERR_ARG, "%s: num_frames %d outside 1..%d", fn, num_frames, TG_SCAN_MAX_FRAMES);
    if (num_points < 1 || num_points > TG_SCAN_MAX_POINTS)
        return fail(TG_ERR_ARG, "%s: num_points %d outside 1..%d", fn, num_points, TG_SCAN_MAX_POINTS);
    tg::ScanArgs sa{};
    if (int rc = check_link_frames(fn, "frame", frames, num_frames, -1, sa.f)) return rc;
    const tg_scan_params &p = *params;
    if (p.surface != TG_SCAN_SURFACE && p.surface != TG_SCAN_CELL)
        return fail(TG_ERR_ARG, "%s: surface %d is neither TG_SCAN_SURFACE nor TG_SCAN_CELL", fn, p.surface);
    if (p.align != TG_SCAN_YAW && p.align != TG_SCAN_WORLD && p.align != TG_SCAN_LINK)
        return fail(TG_ERR_ARG, "%s: align %d is none of TG_SCAN_YAW, TG_SCAN_WORLD, TG_SCAN_LINK", fn, p.align);
    if (p.relative != 0) {
        if (!std::isfinite(p.bias) || !std::isfinite(p.scale))
            return fail(TG_ERR_ARG, "%s: relative with a non-finite bias %g or scale %g", fn, (double)p.bias,
                        (double)p.scale);
        if (!(p.lo <= p.hi))
            return fail(TG_ERR_ARG, "%s: relative needs lo <= hi, got %g and %g", fn, (double)p.lo, (double)p.hi);
    }
    if (normals && p.surface == TG_SCAN_CELL)
        return fail(TG_ERR_ARG, "%s: TG_SCAN_CELL has no normals: normals must be null", fn);
    if (!heights && !normals) return fail(TG_ERR_ARG, "%s: heights and normals are both null", fn);
    if (!s) return fail(TG_ERR_ARG, "%s: null tg_sim", fn);
    if (int rc = check_link_frames(fn, "frame", frames, num_frames, s->L)) return rc;
    sa.F = num_frames;
    sa.P = num_points;
    sa.p = p;
    heightfield_args(s, sa);
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_height_scan(s->hash, s->root, s->dof, points, (int)s->N, sa, heights, normals, s->stream))
        return fail(rc, "%s: launch failed", fn);
    return TG_OK;
}

int tg_imu(tg_sim *s, const tg_contact_frame *sensors, int32_t num_sensors, const tg_imu_params *params,
           const float *bias, const int64_t *reset, float *history, float *out) {
    const char *fn = "tg_imu";
    // everything that can be judged without the sim first, then the sim, then the links against its model
    if (!sensors) return fail(TG_ERR_ARG, "%s: null sensors", fn);
    if (!params) return fail(TG_ERR_ARG, "%s: null params", fn);
    if (!out) return fail(TG_ERR_ARG, "%s: null out", fn);
    if (num_sensors < 1 || num_sensors > TG_IMU_MAX_SENSORS)
        return fail(TG_ERR_ARG, "%s: num_sensors %d outside 1..%d", fn, num_sensors, TG_IMU_MAX_SENSORS);
    tg::ImuArgs ia{};
    if (int rc = check_link_frames(fn, "sensor", sensors, num_sensors, -1, ia.s)) return rc;
    const tg_imu_params &p = *params;
    if (!std::isfinite(p.gyro_noise) || p.gyro_noise < 0.f)
        return fail(TG_ERR_ARG, "%s: gyro_noise %g is not a finite number >= 0", fn, (double)p.gyro_noise);
    if (!std::isfinite(p.accel_noise) || p.accel_noise < 0.f)
        return fail(TG_ERR_ARG, "%s: accel_noise %g is not a finite number >= 0", fn, (double)p.accel_noise);
    if (history && !(std::isfinite(p.dt) && p.dt > 0.f))
        return fail(TG_ERR_ARG, "%s: history with a dt %g that is not a finite number > 0", fn, (double)p.dt);
    if (!s) return fail(TG_ERR_ARG, "%s: null tg_sim", fn);
    if (int rc = check_link_frames(fn, "sensor", sensors, num_sensors, s->L)) return rc;
    ia.S = num_sensors;
    memcpy(ia.g, s->gravity, sizeof ia.g);   // the gravity of this moment
    ia.dt = p.dt;
    ia.gyro_noise = p.gyro_noise;
    ia.accel_noise = p.accel_noise;
    ia.k0 = (uint32_t)p.seed;
    ia.k1 = (uint32_t)(p.seed >> 32);
    ia.c_lo = (uint32_t)p.counter;
    ia.c_hi = (uint32_t)(p.counter >> 32);
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_imu(s->hash, s->root, s->dof, (int)s->N, ia, bias, reset, history, out, s->stream))
        return fail(rc, "%s: launch failed", fn);
    return TG_OK;
}

int tg_ray_cast(tg_sim *s, const tg_contact_frame *frames, int32_t num_frames, const float *rays, int32_t num_rays,
                const tg_ray_params *params, float *dist, float *normals) {
    const char *fn = "tg_ray_cast";
    // everything that can be judged without the sim first, then the sim, then the links against its model
    if (!frames) return fail(TG_ERR_ARG, "%s: null frames", fn);
    if (!rays) return fail(TG_ERR_ARG, "%s: null rays", fn);
    if (!params) return fail(TG_ERR_ARG, "%s: null params", fn);
    if (!dist && !normals) return fail(TG_ERR_ARG, "%s: dist and normals are both null", fn);
    if (num_frames < 1 || num_frames > TG_RAY_MAX_FRAMES)
        return fail(TG_ERR_ARG, "%s: num_frames %d outside 1..%d", fn, num_frames, TG_RAY_MAX_FRAMES);
    if (num_rays < 1 || num_rays > TG_RAY_MAX_RAYS)
        return fail(TG_ERR_ARG, "%s: num_rays %d outside 1..%d", fn, num_rays, TG_RAY_MAX_RAYS);
    tg::RayArgs ra{};
    if (int rc = check_link_frames(fn, "frame", frames, num_frames, -1, ra.f)) return rc;
    const tg_ray_params &p = *params;
    if (p.align != TG_RAY_LINK && p.align != TG_RAY_YAW && p.align != TG_RAY_WORLD)
        return fail(TG_ERR_ARG, "%s: align %d is none of TG_RAY_LINK, TG_RAY_YAW, TG_RAY_WORLD", fn, p.align);
    if (!(std::isfinite(p.max_range) && p.max_range > 0.f))
        return fail(TG_ERR_ARG, "%s: max_range %g is not a finite number > 0", fn, (double)p.max_range);
    if (!s) return fail(TG_ERR_ARG, "%s: null tg_sim", fn);
    if (int rc = check_link_frames(fn, "frame", frames, num_frames, s->L)) return rc;
    ra.F = num_frames;
    ra.R = num_rays;
    ra.align = p.align;
    ra.max_range = p.max_range;
    heightfield_args(s, ra);
    ra.hf_zcap = s->hf_zcap;
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_ray_cast(s->hash, s->root, s->dof, rays, (int)s->N, ra, dist, normals, s->stream))
        return fail(rc, "%s: launch failed", fn);
    return TG_OK;
}

int tg_proximity(tg_sim *s, const tg_capsule *capsules, int32_t num_capsules, const int32_t *pairs, int32_t num_pairs,
                 const tg_proximity_params *params, float *dist, float *witness, float *summary) {
    const char *fn = "tg_proximity";
    // in the header's order: the sim, the pointers, the counts, the capsules, the pairs, the margin, the outputs
    if (!s) return fail(TG_ERR_ARG, "%s: null tg_sim", fn);
    if (!capsules) return fail(TG_ERR_ARG, "%s: null capsules", fn);
    if (!pairs) return fail(TG_ERR_ARG, "%s: null pairs", fn);
    if (!params) return fail(TG_ERR_ARG, "%s: null params", fn);
    if (num_capsules < 1 || num_capsules > TG_PROX_MAX_CAPSULES)
        return fail(TG_ERR_ARG, "%s: num_capsules %d outside 1..%d", fn, num_capsules, TG_PROX_MAX_CAPSULES);
    if (num_pairs < 1 || num_pairs > TG_PROX_MAX_PAIRS)
        return fail(TG_ERR_ARG, "%s: num_pairs %d outside 1..%d", fn, num_pairs, TG_PROX_MAX_PAIRS);
    tg::ProxArgs pa{};
    for (int k = 0; k < num_capsules; ++k)
        if (capsules[k].link < 0 || capsules[k].link >= s->L)
            return fail(TG_ERR_ARG, "%s: capsule %d: link %d outside [0, %d)", fn, k, capsules[k].link, (int)s->L);
    for (int k = 0; k < num_capsules; ++k) {
        const tg_capsule &c = capsules[k];
        for (int i = 0; i < 3; ++i) {
            if (!std::isfinite(c.p0[i])) return fail(TG_ERR_ARG, "%s: capsule %d: p0[%d] is not finite", fn, k, i);
            if (!std::isfinite(c.p1[i])) return fail(TG_ERR_ARG, "%s: capsule %d: p1[%d] is not finite", fn, k, i);
        }
        if (!std::isfinite(c.radius) || c.radius < 0.f)
            return fail(TG_ERR_ARG, "%s: capsule %d: radius %g is not a finite number >= 0", fn, k, (double)c.radius);
        pa.c[k] = c;
    }
    for (int p = 0; p < num_pairs; ++p) {
        const int32_t ia = pairs[2 * p], ib = pairs[2 * p + 1];
        if (ia < 0 || ia >= num_capsules || ib < 0 || ib >= num_capsules)
            return fail(TG_ERR_ARG, "%s: pair %d: (%d, %d) outside [0, %d)", fn, p, ia, ib, num_capsules);
        if (ia == ib) return fail(TG_ERR_ARG, "%s: pair %d: capsule %d with itself", fn, p, ia);
        pa.pair[p][0] = (uint8_t)ia;
        pa.pair[p][1] = (uint8_t)ib;
    }
    if (!std::isfinite(params->margin))
        return fail(TG_ERR_ARG, "%s: margin %g is not finite", fn, (double)params->margin);
    if (!dist && !witness && !summary) return fail(TG_ERR_ARG, "%s: dist, witness and summary are all null", fn);
    pa.C = num_capsules;
    pa.P = num_pairs;
    pa.margin = params->margin;
    DeviceGuard dg(s->device);
    win_touch(s);
    if (int rc = tg::launch_proximity(s->hash, s->root, s->dof, (int)s->N, pa, dist, witness, summary, s->stream))
        return fail(rc, "%s: launch failed", fn);
    return TG_OK;
}

int tg_set_net_contact_force_tensor(tg_sim *s, float *out) {
    if (int rc = check_sim(s)) return rc;
    if (!out) {
        s->cf = nullptr;
        return TG_OK;
    }
    if (tg::jit_has(s->hash))
        return fail(TG_ERR_MODEL,
                    "tg_set_net_contact_force_tensor: the net contact force export exists for compiled-in models "
                    "only, not for a model compiled at run time (tg_model_jit)");
    DeviceGuard dg(s->device);
    win_touch(s);
    // links without a shape are never written by the step kernel: they read 0
    HIPCHK(hipMemsetAsync(out, 0, (size_t)s->N * s->L * 3 * sizeof(float), s->stream));
    s->cf = out;
    return TG_OK;
}

int tg_set_dof_force_tensor(tg_sim *s, float *out) {
    if (int rc = check_sim(s)) return rc;
    if (!out) {
        s->df = nullptr;
        return TG_OK;
    }
    if (tg::jit_has(s->hash))
        return fail(TG_ERR_MODEL,
                    "tg_set_dof_force_tensor: the DOF force export exists for compiled-in models only, not for a "
                    "model compiled at run time (tg_model_jit)");
    DeviceGuard dg(s->device);
    win_touch(s);
    // (the step kernel rewrites every entry, the locked DOFs' zeros included;
    // until the first simulate the tensor reads 0)
    HIPCHK(hipMemsetAsync(out, 0, (size_t)s->N * s->D * sizeof(float), s->stream));
    s->df = out;
    return TG_OK;
}

int tg_set_force_sensor_tensor(tg_sim *s, const tg_contact_frame *sensors, int32_t num_sensors, int32_t space,
                               float *out) {
    const char *fn = "tg_set_force_sensor_tensor";
    if (!s) return fail(TG_ERR_ARG, "%s: null tg_sim", fn);
    if (num_sensors < 0 || num_sensors > TG_FS_MAX_SENSORS)
        return fail(TG_ERR_ARG, "%s: num_sensors %d outside 0..%d", fn, num_sensors, TG_FS_MAX_SENSORS);
    if (num_sensors > 0 && !sensors) return fail(TG_ERR_ARG, "%s: null sensors", fn);
    if (space != TG_ENV_SPACE && space != TG_LOCAL_SPACE)
        return fail(TG_ERR_ARG, "%s: space %d is neither TG_ENV_SPACE nor TG_LOCAL_SPACE", fn, space);
    if (out && num_sensors == 0) return fail(TG_ERR_ARG, "%s: an output tensor with num_sensors 0", fn);
    tg::FsFrames fr{};
    for (int k = 0; k < num_sensors; ++k) {
        const int l = sensors[k].link;
        if (l < 0 || l >= s->L) return fail(TG_ERR_ARG, "%s: sensor %d: link %d outside [0, %d)", fn, k, l, s->L);
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(sensors[k].offset[i]))
                return fail(TG_ERR_ARG, "%s: sensor %d: offset[%d] is not finite", fn, k, i);
        fr.c[k] = sensors[k];
    }
    if (!out || num_sensors == 0) {
        s->fs = nullptr;
        s->fs_frames = tg::FsFrames{};
        return TG_OK;
    }
    if (tg::jit_has(s->hash))
        return fail(TG_ERR_MODEL,
                    "%s: the force sensor export exists for compiled-in models only, not for a model compiled at "
                    "run time (tg_model_jit)", fn);
    fr.n = num_sensors;
    fr.space = space;
    DeviceGuard dg(s->device);
    win_touch(s);
    // sensors on links without a shape, and every sensor of a model without
    // contact rows, are never written by the step kernel: they read 0
    HIPCHK(hipMemsetAsync(out, 0, (size_t)s->N * num_sensors * 6 * sizeof(float), s->stream));
    s->fs = out;
    s->fs_frames = fr;
    return TG_OK;
}

int tg_composite(tg_sim *s, float *out, int32_t recompose) {
    if (int rc = check_sim(s)) return rc;
    if (!out) return fail(TG_ERR_ARG, "tg_composite: null output");
    DeviceGuard dg(s->device);
    if (recompose) {
        HIPCHK(hipMemsetAsync(s->dirty, 1, s->N, s->stream));
        tg::StepArgs a = step_args(s);
        a.cnext = s->ccount + s->list_cur;
        win_touch(s);
        if (int rc = tg::launch_compose_only(s->hash, a, s->stream)) return fail(rc, "compose launch failed");
        s->list_pending = false;
        s->dirty_possible = false;
    }
    HIPCHK(hipMemcpyAsync(out, s->comp, (size_t)s->N * s->KC * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
    return TG_OK;
}

int tg_debug_launch_stats(tg_sim *s, int64_t out[6]) {
    if (int rc = check_sim(s)) return rc;
    if (!out) return fail(TG_ERR_ARG, "tg_debug_launch_stats: null output");
    memcpy(out, s->stats, sizeof s->stats);
    return TG_OK;
}

int tg_set_kernel_timing(tg_sim *s, int32_t period) {
    if (int rc = check_sim(s)) return rc;
    s->timing = period;
    s->timing_count = 0;
    if (s->win.first) {   // an open window is dropped
        s->ev_free.push_back(s->win);
        s->win = {nullptr, nullptr};
    }
    return TG_OK;
}

int tg_read_kernel_timing(tg_sim *s, double *total_ms, int64_t *launches) {
    if (int rc = check_sim(s)) return rc;
    if (!total_ms || !launches) return fail(TG_ERR_ARG, "tg_read_kernel_timing: null argument");
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pend;
    std::vector<int> cnt;
    pend.swap(s->ev_pending);   // every pair leaves the pending list, read or not
    cnt.swap(s->ev_launches);
    for (auto &e : pend) s->ev_free.push_back(e);
    for (size_t i = 0; i < pend.size(); ++i) {
        HIPCHK(hipEventSynchronize(pend[i].second));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, pend[i].first, pend[i].second));
        s->timed_ms += ms;
        s->timed_launches += cnt[i];
    }
    *total_ms = s->timed_ms;
    *launches = s->timed_launches;
    s->timed_ms = 0.0;
    s->timed_launches = 0;
    return TG_OK;
}

int tg_sync(tg_sim *s) {
    if (int rc = check_sim(s)) return rc;
    HIPCHK(hipStreamSynchronize(s->stream));
    int err = 0;
    HIPCHK(hipMemcpy(&err, s->err, sizeof err, hipMemcpyDeviceToHost));
    if (err) {
        HIPCHK(hipMemset(s->err, 0, sizeof err));
        if (err & 2)
            return fail(TG_ERR_STATE, "tg_paper_step: a workgroup of the one-launch step never became resident "
                                      "(reward term 7's batch sum timed out; set TG_PAPER_TWO_LAUNCH=1)");
        return fail(TG_ERR_STATE,
                    "a locked dof was given a [lower, upper] window wider than %g: locked joints are merged into "
                    "their parent's body in this model and stay rigid at the window centre (build the model "
                    "with that joint free instead)", (double)TG_LOCK_WINDOW_MAX);
    }
    return TG_OK;
}

void tg_philox4x32_10(const uint32_t *ctr, const uint32_t *key, uint32_t *out) {
    const tg::U4 r = tg::philox(tg::U4{ctr[0], ctr[1], ctr[2], ctr[3]}, key[0], key[1]);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

int tg_rng_fill(tg_sim *s, int32_t kind, uint64_t seed, uint64_t counter, float *out, int32_t n) {
    if (int rc = check_sim(s)) return rc;
    if (n < 0 || (n > 0 && !out)) return fail(TG_ERR_ARG, "tg_rng_fill: bad output");
    if (kind < 0 || kind > 2) return fail(TG_ERR_ARG, "tg_rng_fill: unknown kind %d", kind);
    win_touch(s);
    if (int rc = tg::launch_rng_fill(kind, seed, counter, out, n, s->stream)) return fail(rc, "rng launch failed");
    return TG_OK;
}

int tg_debug_fill_lds(tg_sim *s, uint32_t pattern) {
    if (int rc = check_sim(s)) return rc;
    win_touch(s);
    if (int rc = tg::launch_fill_lds(pattern, s->stream)) return fail(rc, "LDS fill launch failed");
    return TG_OK;
}

int tg_gogoro_pre_physics(tg_sim *s, const tg_gogoro_params *p, const tg_gogoro_buffers *b, const float *actions,
                          const float *pre_draws, uint64_t counter) {
    if (int rc = check_sim(s)) return rc;
    s->dirty_possible = true;
    if (!p || !b || !actions) return fail(TG_ERR_ARG, "tg_gogoro_pre_physics: null argument");
    if (p->num_envs != s->N || p->num_dof != s->D) return fail(TG_ERR_ARG, "gogoro params do not match the sim");
    win_touch(s);
    if (int rc = tg::launch_gogoro_pre(*p, *b, actions, pre_draws, counter, s->stream)) return fail(rc, "launch failed");
    return TG_OK;
}

int tg_gogoro_step(tg_sim *s, const tg_gogoro_params *p, const tg_gogoro_buffers *b, const float *actions,
                   int32_t n_simulate, const float *pre_draws, const float *reset_draws, const float *obs_draws,
                   const float *speed_draws, const float *yaw_draws, uint64_t counter_pre, uint64_t counter_post) {
    if (int rc = check_sim(s)) return rc;
    if (!p || !b || !actions) return fail(TG_ERR_ARG, "tg_gogoro_step: null argument");
    if (p->num_envs != s->N || p->num_dof != s->D) return fail(TG_ERR_ARG, "gogoro params do not match the sim");
    if (n_simulate < 1) return fail(TG_ERR_ARG, "tg_gogoro_step: n_simulate %d < 1", n_simulate);
    if ((speed_draws == nullptr) != (yaw_draws == nullptr))
        return fail(TG_ERR_ARG, "speed_draws and yaw_draws must both be given or both be NULL");
    for (int i = 0; i < n_simulate; ++i) {
        tg::StepArgs a = step_args(s);
        if (i == 0) {   // pre_physics_step fused into the first compose launch
            tg::GogoroPre &g = a.gp;
            g.actions = actions;
            g.action_history = b->action_history;
            g.curent_command = b->curent_command;
            g.pos_target = b->pos_target;
            g.vel_target = b->vel_target;
            g.steer_offsets = b->steer_offsets;
            g.curent_speed = b->curent_speed;
            g.pre_draws = pre_draws;
            g.clip_actions = p->clip_actions;
            g.max_steering_change = p->max_steering_change;
            g.max_steering = p->max_steering;
            g.noise_mean = p->steering_action_noise[0];
            g.noise_std = p->steering_action_noise[1];
            g.dof_steer = p->dof_steer;
            g.dof_rear = p->dof_rear;
            g.absolute_steer = p->absolute_steer;
            g.k0 = (uint32_t)p->seed;
            g.k1 = (uint32_t)(p->seed >> 32);
            g.c_lo = (uint32_t)counter_pre;
            g.c_hi = (uint32_t)(counter_pre >> 32);
        }
        if (i == n_simulate - 1 && !s->post_unfused) {   // post-physics fused into the last step kernel
            // models whose resets only move translating locks (the seat chain)
            // update their composites in the epilogue; others list their resets
            const bool inplace = tg::model_info(s->hash).tl > 0 && !s->no_inplace;
            const tg::GogoroPostArgs gp{*p, *b, (uint32_t)counter_post, (uint32_t)(counter_post >> 32),
                                        inplace ? nullptr : s->clist + (size_t)s->list_cur * s->N,
                                        inplace ? nullptr : s->ccount + s->list_cur, inplace ? 1 : 0,
                                        reset_draws, obs_draws, speed_draws, yaw_draws};
            // one launch: the pre-physics too runs in the step kernel
            a.gp_in_step = (n_simulate == 1 && !s->pre_in_compose) ? 1 : 0;
            tg::StepPost post;
            post.gogoro = &gp;
            const int rc = simulate_args(s, a, post);
            if (rc == 0) return TG_OK;
            if (rc < 0) return rc;
            a.gp_in_step = 0;   // no fused instantiation: the prologue rides in compose
        }
        if (int rc = simulate_args(s, a)) return rc;
    }
    win_touch(s);
    if (int rc = tg::launch_gogoro_post(*p, *b, reset_draws, obs_draws, speed_draws, yaw_draws, counter_post,
                                        s->stream))
        return fail(rc, "launch failed");
    s->dirty_possible = true;   // the separate post kernel's resets mark envs dirty
    return TG_OK;
}

int tg_gogoro_post_physics(tg_sim *s, const tg_gogoro_params *p, const tg_gogoro_buffers *b, const float *reset_draws,
                           const float *obs_draws, const float *speed_draws, const float *yaw_draws, uint64_t counter) {
    if (int rc = check_sim(s)) return rc;
    s->dirty_possible = true;
    if (!p || !b) return fail(TG_ERR_ARG, "tg_gogoro_post_physics: null argument");
    if (p->num_envs != s->N || p->num_dof != s->D) return fail(TG_ERR_ARG, "gogoro params do not match the sim");
    if ((speed_draws == nullptr) != (yaw_draws == nullptr))
        return fail(TG_ERR_ARG, "speed_draws and yaw_draws must both be given or both be NULL");
    win_touch(s);
    if (int rc = tg::launch_gogoro_post(*p, *b, reset_draws, obs_draws, speed_draws, yaw_draws, counter, s->stream))
        return fail(rc, "launch failed");
    return TG_OK;
}

int tg_gogoro_reset_idx(tg_sim *s, const tg_gogoro_params *p, const tg_gogoro_buffers *b, const int32_t *ids,
                        int32_t n, const float *reset_draws, uint64_t counter) {
    if (int rc = check_sim(s)) return rc;
    s->dirty_possible = true;
    if (int rc = check_ids(s, ids, n)) return rc;
    if (!p || !b) return fail(TG_ERR_ARG, "tg_gogoro_reset_idx: null argument");
    if (p->num_envs != s->N || p->num_dof != s->D) return fail(TG_ERR_ARG, "gogoro params do not match the sim");
    win_touch(s);
    if (int rc = tg::launch_gogoro_reset_idx(*p, *b, ids, n, reset_draws, counter, s->stream))
        return fail(rc, "launch failed");
    return TG_OK;
}

static int check_walk(tg_sim *s, const tg_walk_params *p, const tg_walk_buffers *b) {
    if (int rc = check_sim(s)) return rc;
    if (!p || !b) return fail(TG_ERR_ARG, "walk: null argument");
    if (p->num_envs != s->N || p->num_dof != s->D || p->num_groups != s->G)
        return fail(TG_ERR_ARG, "walk params do not match the sim (N %d/%d, D %d/%d, G %d/%d)", p->num_envs, s->N,
                    p->num_dof, s->D, p->num_groups, s->G);
    if (p->num_dof > TG_WALK_MAX_DOF) return fail(TG_ERR_ARG, "walk: num_dof %d > %d", p->num_dof, TG_WALK_MAX_DOF);
    if (p->num_obs != TG_WALK_NUM_OBS_BASE + 3 * p->num_dof) return fail(TG_ERR_ARG, "walk: num_obs mismatch");
    return 0;
}

int tg_walk_pre_physics(tg_sim *s, const tg_walk_params *p, const tg_walk_buffers *b, const float *actions) {
    if (int rc = check_walk(s, p, b)) return rc;
    if (!actions) return fail(TG_ERR_ARG, "walk: null actions");
    win_touch(s);
    if (int rc = tg::launch_walk_pre(*p, *b, actions, s->stream)) return fail(rc, "launch failed");
    return TG_OK;
}

// pre_physics_step as the prologue of a simulate (StepArgs pm_*)
static void walk_pre_args(tg::StepArgs &a, const tg_walk_params *p, const tg_walk_buffers *b, const float *actions) {
    a.pm_actions = actions;
    a.pm_act_out = b->actions;
    a.pm_tgt_out = b->pos_target;
    a.pm_scale = p->action_scale;
    a.pm_clip = p->clip_actions;
    for (int d = 0; d < p->num_dof; ++d) a.pm_default[d] = p->default_pos[d];
}

int tg_walk_step(tg_sim *s, const tg_walk_params *p, const tg_walk_buffers *b, const float *actions,
                 int32_t n_simulate, const float *reset_draws, const float *push_draws, uint64_t counter) {
    if (int rc = check_walk(s, p, b)) return rc;
    if (!actions || !b->actions || !b->pos_target) return fail(TG_ERR_ARG, "walk step: null actions / targets");
    if (n_simulate < 1) return fail(TG_ERR_ARG, "walk step: n_simulate %d < 1", n_simulate);
    if (p->num_dof > tg::TG_PM_MAX_DOF) return fail(TG_ERR_ARG, "walk step: num_dof %d > %d", p->num_dof, tg::TG_PM_MAX_DOF);
    if (b->body_force) {   // pre_physics_step: apply_rigid_body_force_tensors(body_force)
        if (int rc = copy_full(s, s->force, b->body_force, (size_t)s->N * s->G * 6)) return rc;
        s->forces_pending = true;
        s->rbf_pending = false;
        s->rbf_prereduced = false;
    }
    if (n_simulate == 1 && !s->walk_unfused && !s->pre_in_compose) {
        // one launch per step: pre-physics (drive targets formed from the
        // actions where pass 2a loads them), physics and post-physics all in
        // the step kernel; the compose launch runs only if an env may be dirty
        tg::StepArgs a = step_args(s);
        walk_pre_args(a, p, b, actions);
        a.pm_in_step = 1;
        const tg::WalkPostArgs wp{*p, *b, reset_draws, push_draws, (uint32_t)counter, (uint32_t)(counter >> 32)};
        tg::StepPost post;
        post.walk = &wp;
        const int rc = simulate_args(s, a, post);
        if (rc <= 0) return rc;
        // rc == 1: no fused instantiation for this model / ground -- the general path below
    }
    for (int i = 0; i < n_simulate; ++i) {
        tg::StepArgs a = step_args(s);
        if (i == 0) walk_pre_args(a, p, b, actions);   // pre_physics_step fused into the first compose launch
        if (i == n_simulate - 1 && !s->walk_unfused) {   // post-physics fused into the last step kernel
            const tg::WalkPostArgs wp{*p, *b, reset_draws, push_draws, (uint32_t)counter, (uint32_t)(counter >> 32)};
            tg::StepPost post;
            post.walk = &wp;
            const int rc = simulate_args(s, a, post);
            if (rc == 0) return TG_OK;
            if (rc < 0) return rc;
        }
        if (int rc = simulate_args(s, a)) return rc;
    }
    win_touch(s);
    if (int rc = tg::launch_walk_post(*p, *b, reset_draws, push_draws, counter, s->stream))
        return fail(rc, "launch failed");
    return TG_OK;
}

int tg_walk_post_physics(tg_sim *s, const tg_walk_params *p, const tg_walk_buffers *b, const float *reset_draws,
                         const float *push_draws, uint64_t counter) {
    if (int rc = check_walk(s, p, b)) return rc;
    win_touch(s);
    if (int rc = tg::launch_walk_post(*p, *b, reset_draws, push_draws, counter, s->stream))
        return fail(rc, "launch failed");
    return TG_OK;
}

int tg_walk_reset_idx(tg_sim *s, const tg_walk_params *p, const tg_walk_buffers *b, const int32_t *ids, int32_t n,
                      const float *reset_draws, uint64_t counter) {
    if (int rc = check_walk(s, p, b)) return rc;
    if (int rc = check_ids(s, ids, n)) return rc;
    win_touch(s);
    if (int rc = tg::launch_walk_reset_idx(*p, *b, ids, n, reset_draws, counter, s->stream))
        return fail(rc, "launch failed");
    return TG_OK;
}

static int check_paper(tg_sim *s, const tg_paper_params *p, const tg_paper_buffers *b) {
    if (int rc = check_sim(s)) return rc;
    if (!p || !b) return fail(TG_ERR_ARG, "paper: null argument");
    if (p->num_envs != s->N || p->num_dof != s->D || p->num_groups != s->G)
        return fail(TG_ERR_ARG, "paper params do not match the sim (N %d/%d, D %d/%d, G %d/%d)", p->num_envs, s->N,
                    p->num_dof, s->D, p->num_groups, s->G);
    const int dofs[5] = {p->dof_steer, p->dof_rear, p->dof_base_x, p->dof_base_y, p->dof_base_z};
    for (int d : dofs)
        if (d < 0 || d >= p->num_dof) return fail(TG_ERR_ARG, "paper: dof index %d out of range", d);
    if ((int)p->command_delay[1] != TG_PAPER_CMD_HIST)
        return fail(TG_ERR_ARG, "paper: command_delay[1] must be %d", TG_PAPER_CMD_HIST);
    if (!b->scratch || !b->buffer_obs || !b->buffer_obs_noisy || !b->obs_buf)
        return fail(TG_ERR_ARG, "paper: missing history / scratch buffers");
    if (p->push_robot && p->push_interval <= 0) return fail(TG_ERR_ARG, "paper: push_interval must be > 0");
    return 0;
}

int tg_paper_pre_physics(tg_sim *s, const tg_paper_params *p, const tg_paper_buffers *b, const float *actions,
                         uint64_t counter) {
    (void)counter;
    if (int rc = check_paper(s, p, b)) return rc;
    if (!actions) return fail(TG_ERR_ARG, "paper: null actions");   // (targets / history only: nothing to compose)
    win_touch(s);
    if (int rc = tg::launch_paper_pre(*p, *b, actions, s->stream)) return fail(rc, "launch failed");
    return TG_OK;
}

// tg_paper_step in one launch: the pre-physics, the simulate and the
// post-physics (PaperPost) in the step kernel.  Reward term 7's batch sum is
// exchanged inside the launch, so every workgroup must be resident at once:
// one workgroup per CU at most (TG_PAPER_T7_BLK envs each).  Returns 1 when
// the launch does not apply (model, ground, batch size, residency): the
// caller takes the two-launch path.
static tg::PaperPre paper_pre_args(const tg_paper_params *p, const tg_paper_buffers *b, const float *actions) {
    tg::PaperPre q{};
    q.actions = actions;
    q.command_history = b->command_history;
    q.steer_delay = b->steer_delay;
    q.curent_speed = b->curent_speed;
    q.curent_command = b->curent_command;
    q.pos_target = b->pos_target;
    q.vel_target = b->vel_target;
    q.max_steering = p->max_steering;
    q.use_steer_delay = p->use_steer_delay;
    q.dof_steer = p->dof_steer;
    q.dof_rear = p->dof_rear;
    return q;
}
static int paper_one_launch(tg_sim *s, const tg_paper_params *p, const tg_paper_buffers *b, const float *actions,
                            uint64_t counter) {
    if (s->paper_two_launch || s->pre_in_compose || s->paper_finish_launch || s->no_inplace || s->hf_rows > 0 ||
        (b->rb_forces && s->paper_rb_launch) || !(tg::model_info(s->hash).fused & 4) || tg::model_info(s->hash).tl <= 0)
        return 1;
    const int epb = tg::model_info(s->hash).epb;
    if (epb != TG_PAPER_T7_BLK || s->N % epb != 0) return 1;
    if (s->num_cus == 0) {
        DeviceGuard dg(s->device);
        HIPCHK(hipDeviceGetAttribute(&s->num_cus, hipDeviceAttributeMultiprocessorCount, s->device));
    }
    const int nblk = s->N / epb;
    if (nblk > s->num_cus || nblk > TG_PAPER_T7_THREADS) return 1;
    if (!s->t7cnt) {
        DeviceGuard dg(s->device);
        if (s->alloc(&s->t7cnt, 1)) return TG_ERR_HIP;
        s->t7_total = 0;
    }
    tg::StepArgs a = step_args(s);
    a.pp = paper_pre_args(p, b, actions);
    a.pp_in_step = 1;
    a.pp.buffer_obs = b->buffer_obs;
    a.pp.reset_buf = b->reset_buf;
    a.pp.t7 = reinterpret_cast<double *>(b->scratch);   // (N floats hold N / 16 doubles)
    const bool rb = b->rb_forces != nullptr;
    const tg::PaperPostArgs pa{*p, *b, (uint32_t)counter, (uint32_t)(counter >> 32), rb ? s->force : nullptr,
                               s->t7cnt, s->t7_total + (unsigned)nblk, nblk};
    tg::StepPost post;
    post.paper = &pa;
    if (int rc = simulate_args(s, a, post)) return rc < 0 ? rc : 1;
    s->t7_total += (unsigned)nblk;   // (the launch adds nblk arrivals)
    if (rb) {   // the next simulate's rigid-body forces, reduced already
        s->rbf_f = b->rb_forces;
        s->rbf_t = nullptr;
        s->rbf_space = TG_ENV_SPACE;
        s->rbf_pending = false;
        s->rbf_prereduced = true;
        s->forces_pending = true;
    }
    return TG_OK;
}

int tg_paper_step(tg_sim *s, const tg_paper_params *p, const tg_paper_buffers *b, const float *actions,
                  int32_t n_simulate, uint64_t counter) {
    if (int rc = check_paper(s, p, b)) return rc;
    if (!actions) return fail(TG_ERR_ARG, "paper: null actions");
    if (n_simulate < 1) return fail(TG_ERR_ARG, "tg_paper_step: n_simulate %d < 1", n_simulate);
    if (n_simulate == 1) {
        const int rc = paper_one_launch(s, p, b, actions, counter);
        if (rc != 1) return rc;
    }
    bool fin = false;
    for (int i = 0; i < n_simulate; ++i) {
        tg::StepArgs a = step_args(s);
        if (i == 0) {   // pre_physics_step as the first compose launch's prologue
            tg::PaperPre &q = a.pp;
            q = paper_pre_args(p, b, actions);
            // in the step kernel itself when it is the only simulate and the
            // model's kernel has the pre-physics slots; else the compose prologue
            // (FUSED bit 4: the bit the step kernel tests before it runs the
            // paper pre-physics and forms the term-7 partials)
            a.pp_in_step = (n_simulate == 1 && (tg::model_info(s->hash).fused & 4) && !s->pre_in_compose) ? 1 : 0;
            // the step kernel also forms reward term 7's partials, so the post
            // launch finishes the batch itself (no finish launch)
            if (a.pp_in_step && !s->paper_finish_launch && p->num_envs % 8 == 0) {   // 8: PAPER_EPW
                q.buffer_obs = b->buffer_obs;
                q.reset_buf = b->reset_buf;
                q.t7 = reinterpret_cast<double *>(b->scratch);   // (N floats hold N / 16 doubles)
                fin = true;
            }
        }
        if (int rc = simulate_args(s, a)) return rc < 0 ? rc : fail(TG_ERR_STATE, "no step kernel for this model");
    }
    bool inplace = false, rb_done = false;
    const bool rb_fuse = b->rb_forces && !s->paper_rb_launch;
    win_touch(s);
    if (int rc = tg::launch_paper_post(*p, *b, nullptr, nullptr, nullptr, nullptr, nullptr, counter, s->stream,
                                       s->hash, s->no_inplace ? nullptr : s->comp, &inplace, fin,
                                       rb_fuse ? s->force : nullptr, &rb_done))
        return fail(rc, "launch failed");
    if (b->rb_forces) {   // the next simulate's rigid-body forces: reduced already, or pending as if applied now
        s->rbf_f = b->rb_forces;
        s->rbf_t = nullptr;
        s->rbf_space = TG_ENV_SPACE;
        s->rbf_pending = !rb_done;
        s->rbf_prereduced = rb_done;
        s->forces_pending = true;
    }
    // the post kernel's resets either update the seat composites in place or
    // mark their envs for the next compose
    if (!inplace) s->dirty_possible = true;
    return TG_OK;
}

int tg_paper_post_physics(tg_sim *s, const tg_paper_params *p, const tg_paper_buffers *b, const float *reset_draws,
                          const float *noise_draws, const float *speed_draws, const float *yaw_draws,
                          const float *push_draws, uint64_t counter) {
    if (int rc = check_paper(s, p, b)) return rc;
    const bool dirty_before = s->dirty_possible;
    s->dirty_possible = true;
    bool inplace = false;
    win_touch(s);
    if (int rc = tg::launch_paper_post(*p, *b, reset_draws, noise_draws, speed_draws, yaw_draws, push_draws, counter,
                                       s->stream, s->hash, s->no_inplace ? nullptr : s->comp, &inplace))
        return fail(rc, "launch failed");
    if (inplace) s->dirty_possible = dirty_before;
    return TG_OK;
}

int tg_paper_reset_idx(tg_sim *s, const tg_paper_params *p, const tg_paper_buffers *b, const int32_t *ids, int32_t n,
                       const float *reset_draws, uint64_t counter) {
    if (int rc = check_paper(s, p, b)) return rc;
    s->dirty_possible = true;
    if (int rc = check_ids(s, ids, n)) return rc;
    win_touch(s);
    if (int rc = tg::launch_paper_reset_idx(*p, *b, ids, n, reset_draws, counter, s->stream))
        return fail(rc, "launch failed");
    return TG_OK;
}

}  // extern "C"
