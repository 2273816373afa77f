// The ground surface of tg_set_heightfield, shared by the step kernel's contact
// rows (step_par.h) and the height scan (articulation_kernels.h
// height_scan_kernel): one definition, so that what a scan reports is what the
// contacts feel.
#pragma once
#include <hip/hip_runtime.h>

#include "tg_math.h"

namespace tg {

// Ground surface under world (x, y): the heightfield trimesh of
// tg_set_heightfield (vertex (i,j) at (ox + i hs, oy + j hs, vs h[i][j]);
// cell triangles (i,j)-(i+1,j+1)-(i,j+1) for fv >= fu and
// (i,j)-(i+1,j)-(i+1,j+1) for fu >= fv) or the z = 0 plane, whichever is
// higher.  Returns the height, the unit normal in n and whether the terrain
// is the surface.  oracle/physics_ref.c ground_at is the same function.
// A: any argument block with the heightfield members of StepArgs (hf, hf_rows,
// hf_cols, hf_hs, hf_vs, hf_ox, hf_oy); a.hf is not null.
template <class A>
__device__ __forceinline__ float ground_at(const A &a, float x, float y, V3 &n, bool &on_hf) {
    n = v3(0, 0, 1);
    on_hf = false;
    const float u = (x - a.hf_ox) / a.hf_hs, v = (y - a.hf_oy) / a.hf_hs;
    if (!(u >= 0.f && v >= 0.f && u <= (float)(a.hf_rows - 1) && v <= (float)(a.hf_cols - 1))) return 0.f;
    const int i = min((int)u, a.hf_rows - 2), j = min((int)v, a.hf_cols - 2);
    const float fu = u - (float)i, fv = v - (float)j;
    const float *r0 = a.hf + (size_t)i * a.hf_cols + j, *r1 = r0 + a.hf_cols;
    const float h00 = a.hf_vs * r0[0], h01 = a.hf_vs * r0[1], h10 = a.hf_vs * r1[0], h11 = a.hf_vs * r1[1];
    float H, gx, gy;
    if (fu >= fv) { gx = h10 - h00; gy = h11 - h10; H = h00 + fu * gx + fv * gy; }
    else          { gx = h11 - h01; gy = h01 - h00; H = h00 + fu * gx + fv * gy; }
    if (!(H > 0.f)) return 0.f;
    gx /= a.hf_hs;
    gy /= a.hf_hs;
    const float inv = 1.f / sqrtf(gx * gx + gy * gy + 1.f);
    n = v3(-gx * inv, -gy * inv, inv);
    on_hf = true;
    return H;
}

}  // namespace tg
