// The ground surface of tg_set_heightfield, shared by the step kernel's contact
// rows (step_par.h) and the height scan (articulation_kernels.h
// height_scan_kernel): one definition, so that what a scan reports is what the
// contacts feel.  ground_ray casts a ray against the solid under that surface
// (ray_cast_kernel).
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

// Finite, judged by the bits.  On a word loaded from memory the test holds
// whatever the floating-point flags of the unit let the compiler assume about
// NaN and infinity; on a value computed under those flags it may be folded
// away, so a caller that must reject non-finite input tests its loaded words
// (ray_cast_kernel) and says so in ground_ray's ``finite``.
__device__ __forceinline__ bool ground_finite_bits(unsigned u) { return (u & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool ground_finite(float x) { return ground_finite_bits(__float_as_uint(x)); }

// The first point of the ray x(t) = o + t d, t in [0, tmax], in the ground
// solid G = {z <= 0} u {(x, y) on the grid, z <= H(x, y)} (tgsim.h tg_ray_cast;
// H the triangle height of ground_at, the same cell split and fu >= fv rule).
// Returns its t -- tmax exactly on a miss -- and in n the normal there: e_z on
// the plane, the triangle's unit normal, the outward normal of the grid's
// border face, ground_at's normal for a start inside G, 0 on a miss.
//   1  a start inside G is judged by ground_at itself
//   2  the plane candidate t = -o.z / d.z bounds everything after it
//   3  the ray's (x, y), in cells, is clipped to the grid rectangle (slabs; the
//      axis that clips the entry last is the border face entered, x on a tie)
//      and to z <= hf_zcap, above which there is no terrain
//   4  a 2-D DDA over the cells, each cell's exit recomputed from its integer
//      index (no accumulated step); the span in a cell is split at the cell
//      diagonal, and on each piece f(t) = z(t) - H is linear: f <= 0 at the
//      piece's entry is a hit there (the border face, or a rounding leak
//      between neighbouring triangles: testing every entry makes the walk
//      watertight), f <= 0 at its exit a hit at the root of f
// A vertical ray never steps (both exits are at BIG); a ray parallel to an axis
// steps along the other only; a ray along a cell line sits on the upper
// triangle's edge (fu = 0 < fv) and one along a diagonal on the lower triangle
// (fu >= fv), as ground_at decides there.  The walk is bounded by the integer
// counter, rows + cols + 4 cells, and every index is clamped onto the grid; no
// float comparison decides termination alone.  finite: what o and d were
// formed from is finite (a miss otherwise).  A: RayArgs (the heightfield
// members of StepArgs and hf_zcap; a.hf may be null).
template <class A>
__device__ __forceinline__ float ground_ray(const A &a, V3 o, V3 d, float tmax, bool finite, V3 &n) {
    const float BIG = 3.0e38f;
    n = v3(0, 0, 0);
    if (!finite) return tmax;
    // best effort only: on these computed values the test may be folded away under the unit's flags (see
    // ground_finite), and finite input that overflows here is not promised a miss -- the walk below is memory-safe
    // and bounded whatever o and d hold
    if (!(ground_finite(o.x) && ground_finite(o.y) && ground_finite(o.z) && ground_finite(d.x) &&
          ground_finite(d.y) && ground_finite(d.z)))
        return tmax;
    if (d.x == 0.f && d.y == 0.f && d.z == 0.f) return tmax;
    V3 n0 = v3(0, 0, 1);
    float H0 = 0.f;
    if (a.hf) {
        bool on;
        H0 = ground_at(a, o.x, o.y, n0, on);
    }
    if (o.z <= H0) {
        n = n0;
        return 0.f;
    }
    float best = tmax;
    if (d.z < 0.f) {
        const float tp = -o.z / d.z;
        if (tp < best) {
            best = tp;
            n = v3(0, 0, 1);
        }
    }
    if (a.hf) {
        const int rows = a.hf_rows, cols = a.hf_cols;
        const float U0 = (o.x - a.hf_ox) / a.hf_hs, V0 = (o.y - a.hf_oy) / a.hf_hs;
        const float dU = d.x / a.hf_hs, dV = d.y / a.hf_hs;
        const float iu = dU != 0.f ? 1.f / dU : 0.f, iv = dV != 0.f ? 1.f / dV : 0.f;
        float t0 = 0.f, t1 = best;
        int wall = 0;   // the border face the clipped ray enters through: 1 x, 2 y
        if (dU != 0.f) {
            const float ta = (0.f - U0) * iu, tb = ((float)(rows - 1) - U0) * iu;
            const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
            if (lo > t0) { t0 = lo; wall = 1; }
            t1 = fminf(t1, hi);
        } else if (!(U0 >= 0.f && U0 <= (float)(rows - 1))) {
            t1 = -1.f;
        }
        if (dV != 0.f) {
            const float ta = (0.f - V0) * iv, tb = ((float)(cols - 1) - V0) * iv;
            const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
            if (lo > t0) { t0 = lo; wall = 2; }
            t1 = fminf(t1, hi);
        } else if (!(V0 >= 0.f && V0 <= (float)(cols - 1))) {
            t1 = -1.f;
        }
        if (d.z < 0.f) {
            const float tz = (a.hf_zcap - o.z) / d.z;
            if (tz > t0) { t0 = tz; wall = 0; }
        } else if (d.z > 0.f) {
            t1 = fminf(t1, (a.hf_zcap - o.z) / d.z);
        } else if (o.z > a.hf_zcap) {
            t1 = -1.f;
        }
        if (t0 < t1) {
            const float Ue = U0 + t0 * dU, Ve = V0 + t0 * dV;
            // clamped as a float first, so that the conversion sees a value on the grid, and again as an integer
            int i = min(max((int)fminf(fmaxf(floorf(Ue), 0.f), (float)(rows - 2)), 0), rows - 2);
            int j = min(max((int)fminf(fmaxf(floorf(Ve), 0.f), (float)(cols - 2)), 0), cols - 2);
            const int si = dU > 0.f ? 1 : -1, sj = dV > 0.f ? 1 : -1;
            const float g1 = dU - dV, ig = g1 != 0.f ? 1.f / g1 : 0.f;
            float tc = t0;
            const int budget = rows + cols + 4;
            for (int k = 0; k < budget; ++k) {
                const float tU = dU != 0.f ? ((float)(i + (si > 0 ? 1 : 0)) - U0) * iu : BIG;
                const float tV = dV != 0.f ? ((float)(j + (sj > 0 ? 1 : 0)) - V0) * iv : BIG;
                const float tb = fmaxf(fminf(fminf(tU, tV), t1), tc);
                const float *r0 = a.hf + (size_t)i * cols + j, *r1 = r0 + cols;
                const float h00 = a.hf_vs * r0[0], h01 = a.hf_vs * r0[1], h10 = a.hf_vs * r1[0],
                            h11 = a.hf_vs * r1[1];
                const float a0 = U0 - (float)i, b0 = V0 - (float)j, g0 = a0 - b0;   // fu - fv = g0 + t g1
                const float td = g1 != 0.f ? -g0 * ig : BIG;
                const bool split = td > tc && td < tb;
                bool hit = false;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (s == 1 && (!split || hit)) break;
                    const float sa = s == 0 ? tc : td, sb = (s == 0 && split) ? td : tb;
                    const bool lower = g0 + (0.5f * (sa + sb)) * g1 >= 0.f;
                    float gx, gy;
                    if (lower) { gx = h10 - h00; gy = h11 - h10; }
                    else       { gx = h11 - h01; gy = h01 - h00; }
                    const float c0 = o.z - (h00 + a0 * gx + b0 * gy), c1 = d.z - (dU * gx + dV * gy);
                    const float fa = c0 + sa * c1, fb = c0 + sb * c1;
                    float th = BIG;
                    bool face = false;
                    if (fa <= 0.f) {
                        th = sa;
                        face = k == 0 && s == 0 && wall != 0;
                    } else if (fb <= 0.f) {
                        th = fminf(fmaxf(-c0 / c1, sa), sb);   // fa > 0 >= fb: c1 < 0
                    }
                    if (th < BIG) {
                        hit = true;
                        if (th < best) {
                            best = th;
                            if (face) {
                                n = wall == 1 ? v3(dU > 0.f ? -1.f : 1.f, 0, 0) : v3(0, dV > 0.f ? -1.f : 1.f, 0);
                            } else {
                                gx /= a.hf_hs;
                                gy /= a.hf_hs;
                                const float inv = 1.f / sqrtf(gx * gx + gy * gy + 1.f);
                                n = v3(-gx * inv, -gy * inv, inv);
                            }
                        }
                    }
                }
                if (hit || !(tb < t1)) break;
                if (tU <= tV) i += si;
                else j += sj;
                if (i < 0 || i > rows - 2 || j < 0 || j > cols - 2) break;
                tc = tb;
            }
        }
    }
    if (!(best < tmax)) {
        n = v3(0, 0, 0);
        return tmax;
    }
    return best;
}

}  // namespace tg
