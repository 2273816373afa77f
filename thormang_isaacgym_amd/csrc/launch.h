// launch.h -- the per-model launch templates of the step path (compose, the
// step kernel, the fused task epilogues), shared by the two units that
// instantiate them: articulation.hip (the scooters and the known-answer
// models) and articulation_tree.hip (the humanoid-size trees, NG >= 16).
// The units differ only in the machine scheduler they are compiled with
// (build_ext.py): each model's step kernel is instantiated in exactly one of
// them, chosen by TG_UNIT_TREE.
#pragma once
#include <type_traits>

namespace tg {

#ifndef TG_UNIT_TREE
#define TG_UNIT_TREE 0
#endif
// a launch_* call for a model the other unit instantiates
constexpr int TG_OTHER_UNIT = -1000;
template <class M> constexpr bool in_unit() { return (M::NG >= 16) == (TG_UNIT_TREE != 0); }

// ---------------------------------------------------------------- dispatch
// compose (dirty envs only), then the tree-parallel LDS-resident step,
// M::EPB envs x M::LPE lanes per workgroup (Thormang: 16 envs, 151 KB of LDS).

// the compose launch before a step kernel: none (no env can be dirty and no
// prologue), the listed envs of the last fused epilogue (compose_list_kernel),
// or every dirty env (compose_kernel)
template <class M> void launch_compose(const StepArgs &a, hipStream_t stream) {
    if (a.skip_compose) return;
    if (a.compose_list) {
        hipLaunchKernelGGL(compose_list_kernel<M>, dim3((a.N + COMPOSE_WPB - 1) / COMPOSE_WPB), dim3(64), 0, stream,
                           a);
    } else {
        hipLaunchKernelGGL(compose_kernel<M>, dim3((a.N + COMPOSE_WPB - 1) / COMPOSE_WPB), dim3(64 * COMPOSE_WPB), 0,
                           stream, a);
        if (a.cuni) {   // shared-cache flag for the step kernels that follow
            (void)hipMemsetD32Async(a.cuni, 1, 1, stream);
            hipLaunchKernelGGL(uniform_check_kernel<M>, dim3(a.N), dim3(64), 0, stream, a);
        }
    }
}

// HF: terrain heightfield present (tg_set_heightfield); the flat-ground
// instantiation keeps the contact normal a compile-time e_z.
template <class M, bool HF, class P>
int launch_par(const StepArgs &a, hipStream_t stream, const typename P::Args &pa) {
    constexpr size_t bytes = ParLayout<M>::template bytes<M::EPB>();
    static_assert(bytes <= 160 * 1024, "LDS budget");
    // the dynamic-LDS attribute is per device: one bit per device of this
    // instantiation, set the first time the kernel launches there (sims on
    // several devices in one process, from any thread)
    static std::atomic<uint64_t> attr_set{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TG_ERR_HIP;
    const uint64_t bit = 1ull << dev;
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
        if (hipFuncSetAttribute((const void *)step_par_kernel<M, M::EPB, HF, P>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
            return TG_ERR_HIP;
        attr_set.fetch_or(bit, std::memory_order_acq_rel);
    }
    hipLaunchKernelGGL((step_par_kernel<M, M::EPB, HF, P>), dim3((a.N + M::EPB - 1) / M::EPB),
                       dim3(M::EPB * M::LPE), bytes, stream, a, pa);
    return 0;
}

// What differs between the variants of the step kernel at launch, per post
// policy P: which models have the instantiation (eligible), whether the
// terrain one exists beside the flat-ground one (HF), what a model without it
// runs instead (Fallback; void: nothing, the call is declined with 1), and the
// run-time test of a call (accepts; false: declined with 1, nothing launched).
struct AnyStep {
    template <class M> static constexpr bool eligible = true;
    static constexpr bool HF = true;
    using Fallback = void;
    template <class M, class A> static bool accepts(const StepArgs &, const A &) { return true; }
};
// the plain step, and the DOF force export (NoPostDF, df [N, ND]; with the
// net contact force export too when its cf is not null): one more pair per
// model, with or without contact rows (a model without any has no contact part)
template <class P> struct StepVariant : AnyStep {};
// the net contact force export (NoPostCF, cf [N, NL, 3]): instantiated beside
// the plain pair for every model with contact rows; a model without any has
// nothing to export and runs the plain kernel (the tensor keeps the zeros it
// was enabled with)
template <> struct StepVariant<NoPostCF> : AnyStep {
    template <class M> static constexpr bool eligible = M::NROWS > 0;
    using Fallback = NoPost;
};
// the force sensor export (NoPostFS, fs [N, S, 6], with cf and df when they
// are not null): for every model with contact rows; launch_step sends a model
// without any down the other exports' path (the tensor keeps its zeros)
template <> struct StepVariant<NoPostFS> : AnyStep {
    template <class M> static constexpr bool eligible = M::NROWS > 0;
};
// the fused walk epilogue is instantiated for the lane-pair (humanoid-size)
// trees on flat ground only
template <> struct StepVariant<WalkPost> : AnyStep {
    template <class M> static constexpr bool eligible = M::PAIR != 0 && M::ND <= 64;
    static constexpr bool HF = false;
    template <class M> static bool accepts(const StepArgs &a, const WalkPostArgs &pa) {
        return !a.hf && pa.p.num_dof == M::ND;
    }
};
// the fused Gogoro epilogue is instantiated for the registered task's model
// (codegen FUSED bit 1), flat ground and terrain
template <> struct StepVariant<GogoroPost> : AnyStep {
    template <class M> static constexpr bool eligible = (M::FUSED & 2) != 0;
    template <class M> static bool accepts(const StepArgs &, const GogoroPostArgs &pa) {
        return pa.p.num_dof == M::ND;
    }
};
// the fused GogoroPaper epilogue (one launch per step): the paper model with
// in-place seat composites (codegen FUSED bit 4), flat ground
template <> struct StepVariant<PaperPost> : AnyStep {
    template <class M>
    static constexpr bool eligible = (M::FUSED & 4) != 0 && M::NTL > 0 && M::LCOM && M::NG <= M::LPE && M::LPE >= 8;
    static constexpr bool HF = false;
    template <class M> static bool accepts(const StepArgs &a, const PaperPostArgs &pa) {
        return !a.hf && pa.p.num_dof == M::ND && a.N % M::EPB == 0;
    }
};

// compose, then model M's step kernel with post policy P; ev_begin / ev_end
// (optional) are recorded around the step kernel itself
template <class M, class P>
int launch_model(const StepArgs &a, const typename P::Args &pa, hipStream_t stream, hipEvent_t ev_begin,
                 hipEvent_t ev_end) {
    using V = StepVariant<P>;
    if constexpr (!in_unit<M>()) {
        return TG_OTHER_UNIT;
    } else if constexpr (!V::template eligible<M>) {
        if constexpr (std::is_void_v<typename V::Fallback>) return 1;
        else return launch_model<M, typename V::Fallback>(a, {}, stream, ev_begin, ev_end);
    } else {
        if (!V::template accepts<M>(a, pa)) return 1;
        launch_compose<M>(a, stream);
        if (ev_begin && hipEventRecord(ev_begin, stream) != hipSuccess) return TG_ERR_HIP;
        int rc;
        if constexpr (V::HF) rc = a.hf ? launch_par<M, true, P>(a, stream, pa) : launch_par<M, false, P>(a, stream, pa);
        else rc = launch_par<M, false, P>(a, stream, pa);
        if (rc) return rc;
        if (ev_end && hipEventRecord(ev_end, stream) != hipSuccess) return TG_ERR_HIP;
        return hipGetLastError() == hipSuccess ? 0 : TG_ERR_HIP;
    }
}

// this unit's dispatch (TG_OTHER_UNIT: a model this unit does not instantiate)
#define TG_U_LAUNCH(MODEL) \
    if (in_unit<MODEL>() && hash == MODEL::hash) return launch_model<MODEL, P>(a, pa, stream, ev_begin, ev_end);
template <class P>
static int unit_launch(uint64_t hash, const StepArgs &a, const typename P::Args &pa, hipStream_t stream,
                       hipEvent_t ev_begin, hipEvent_t ev_end) {
    TG_FOR_EACH_MODEL(TG_U_LAUNCH)
    return TG_OTHER_UNIT;
}
#undef TG_U_LAUNCH

// the humanoid unit's entry (articulation_tree.hip instantiates it for every
// post policy of the list)
#define TG_FOR_EACH_POST(X) X(NoPost) X(NoPostCF) X(NoPostDF) X(NoPostFS) X(WalkPost) X(GogoroPost) X(PaperPost)
template <class P>
int tree_launch(uint64_t hash, const StepArgs &a, const typename P::Args &pa, hipStream_t stream, hipEvent_t ev_begin,
                hipEvent_t ev_end);

}  // namespace tg
