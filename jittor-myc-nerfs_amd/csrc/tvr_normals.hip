// tvr_normals.hip — the normal pass of tvr_render_normals: the march's queue in, one weighted normal per ray out.
//
//   N_i = sum_e w_e n_e,   n_e = v_e / sqrt(max(|v_e|^2, 1e-30)),   v_e = -(g_e * inv_aabb_size),   g_e = tvr_density_gradient's value at the entry's position
// over the ray's appearance samples e (the queue entries {xyz_norm, w} the march wrote, contiguous per ray and in sample order).  The gradient is evaluated by the
// per-point code tvr_density_gradient runs (tvr_gradient.h), so g_e is that call's value bit for bit; TensorBase.surface_normals' arithmetic turns it into n_e.
// Nothing per entry goes to memory: 16 B of queue are read, the gathers hit the density factors (VM: 78 float4 per quad-lane, CP: 18 float4 per group of four
// components), and gradient, unit vector and weighted sum stay in registers.
//
// Work distribution.  A ray's entries are handled by 16 SLOTS; slot q takes entries q, q + 16, q + 32, ... in that order and keeps its own partial sum, and a fixed
// butterfly adds the 16 partial sums at the end: the order of the additions is a function of the ray's entry count alone, so N_i is bit-reproducible and does not
// depend on the batch, on the chunking or on which wave took the ray.
//   VM: a slot is a quad (lane >> 2), the mapping of density_gradient_kernel: 4 lanes x 4 of the 16 channels, quad reduction per entry.  One ray per wave at a time.
//   CP: a slot is a lane (lane & 15), the mapping of cp_density_gradient_kernel: the 16-lane group lane >> 4 takes one ray, four rays per wave at a time.
// Rays carry 0 .. S entries, so the waves of a persistent grid draw TICKETS of NORMALS_TICKET_RAYS consecutive rays from a word of the scratch header (zeroed with
// the header at the start of the call; 40 000 atomics for an 800 x 800 frame).  The entry counts are read from the device (ray_cnt), never by the host.
#include "tvr_device.h"
#include "tvr_kernels.h"
#include "tvr_gradient.h"

#define NORMALS_TICKET_WORD 16           // word of the 64-word scratch header; the march uses words 0, 1, 2 (and 32 in one of its build variants)
#define NORMALS_TICKET_RAYS 16

// TensorBase.surface_normals on one gradient, times the entry's weight, added to the slot's sum (separately rounded fp32 throughout: -ffp-contract=off)
__device__ __forceinline__ void normals_accumulate(const SceneDev &sc, float gx, float gy, float gz, float w, float &nx, float &ny, float &nz)
{
    const float vx = -(gx * sc.inv[0]), vy = -(gy * sc.inv[1]), vz = -(gz * sc.inv[2]);
    const float len = sqrtf(fmaxf((vx * vx + vy * vy) + vz * vz, 1e-30f));
    nx = nx + w * (vx / len);
    ny = ny + w * (vy / len);
    nz = nz + w * (vz / len);
}

template <bool CP>
__global__ __launch_bounds__(256) void normals_kernel(const SceneDev sc, const CpDev cp, const MarchOut mo, const int n_rays, const float3 h, const float3 inv2h,
                                                      float *__restrict__ normal_out, float *__restrict__ acc_out, float *__restrict__ depth_out)
{
    const int lane = threadIdx.x & 63;
    const bool fault = mo.counter[2] != 0u;          // the march raised its fault flag (tile-queue wait): nothing of this call is trustworthy
    const float qnan = __int_as_float(0x7fc00000);
    for (;;) {
        unsigned t = 0u;
        if (lane == 0) t = atomicAdd(mo.counter + NORMALS_TICKET_WORD, 1u);
        t = (unsigned)__shfl((int)t, 0);
        const long long r0 = (long long)t * NORMALS_TICKET_RAYS;
        if (r0 >= (long long)n_rays) break;
        const int r1 = (int)(r0 + NORMALS_TICKET_RAYS < (long long)n_rays ? r0 + NORMALS_TICKET_RAYS : (long long)n_rays);
        if (fault) {
            for (int r = (int)r0 + lane; r < r1; r += 64) {
                normal_out[(size_t)r * 3 + 0] = qnan; normal_out[(size_t)r * 3 + 1] = qnan; normal_out[(size_t)r * 3 + 2] = qnan;
                if (acc_out) acc_out[r] = qnan;
                if (depth_out) depth_out[r] = qnan;
            }
            continue;
        }
        if (!CP) {
            const int slot = lane >> 2, sub = lane & 3;
            for (int r = (int)r0; r < r1; ++r) {                         // wave-uniform: one ray at a time
                const unsigned base = mo.ray_off[r], cnt = mo.ray_cnt[r];
                float nx = 0.0f, ny = 0.0f, nz = 0.0f;
                for (unsigned i = 0; i < cnt; i += 16) {
                    const unsigned e = i + (unsigned)slot;
                    const bool live = e < cnt;                           // (quad-uniform)
                    float f[7];
#pragma unroll
                    for (int j = 0; j < 7; ++j) f[j] = 0.0f;
                    float w = 0.0f;
                    if (live) {
                        const float4 q = mo.q_pos[base + e];             // {xyz_norm, weight}
                        w = q.w;
                        vm_grad_point(sc, q.x, q.y, q.z, h, sub, f);
                    }
#pragma unroll
                    for (int j = 1; j < 7; ++j) {                        // density_gradient_kernel's quad reduction: every lane of the quad ends with the same bits
                        f[j] += __shfl_xor(f[j], 1);
                        f[j] += __shfl_xor(f[j], 2);
                    }
                    if (live) normals_accumulate(sc, (f[1] - f[2]) * inv2h.x, (f[3] - f[4]) * inv2h.y, (f[5] - f[6]) * inv2h.z, w, nx, ny, nz);
                }
#pragma unroll
                for (int off = 4; off < 64; off <<= 1) {                 // the 16 slots' sums, fixed shape
                    nx = nx + __shfl_xor(nx, off);
                    ny = ny + __shfl_xor(ny, off);
                    nz = nz + __shfl_xor(nz, off);
                }
                if (lane == 0) {
                    normal_out[(size_t)r * 3 + 0] = nx; normal_out[(size_t)r * 3 + 1] = ny; normal_out[(size_t)r * 3 + 2] = nz;
                    if (acc_out) acc_out[r] = mo.acc[r];
                }
            }
        } else {
            const int slot = lane & 15, grp = lane >> 4;
            for (int rb = (int)r0; rb < r1; rb += 4) {                   // four rays at a time, one per 16-lane group
                const int r = rb + grp;
                const bool have = r < r1;
                const unsigned base = have ? mo.ray_off[r] : 0u, cnt = have ? mo.ray_cnt[r] : 0u;
                float nx = 0.0f, ny = 0.0f, nz = 0.0f;
                for (unsigned e = (unsigned)slot; e < cnt; e += 16) {
                    const float4 q = mo.q_pos[base + e];
                    float f[7];
                    cp_grad_point(sc, cp, q.x, q.y, q.z, h, f);
                    normals_accumulate(sc, (f[1] - f[2]) * inv2h.x, (f[3] - f[4]) * inv2h.y, (f[5] - f[6]) * inv2h.z, q.w, nx, ny, nz);
                }
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {                 // (outside the divergent loop: all 64 lanes are here)
                    nx = nx + __shfl_xor(nx, off);
                    ny = ny + __shfl_xor(ny, off);
                    nz = nz + __shfl_xor(nz, off);
                }
                if (have && slot == 0) {
                    normal_out[(size_t)r * 3 + 0] = nx; normal_out[(size_t)r * 3 + 1] = ny; normal_out[(size_t)r * 3 + 2] = nz;
                    if (acc_out) acc_out[r] = mo.acc[r];
                }
            }
        }
    }
}

hipError_t launch_normals(const SceneDev &sc, const CpDev *cp, const MarchOut &mo, int n_rays, const float h[3], const float inv2h[3], float *normal_out, float *acc_out,
                          float *depth_out, hipStream_t stream)
{
    // persistent grid of 256-thread blocks, as many per CU as the registers admit (VM: 155 VGPRs, three waves per SIMD; CP: 111, four), never more waves than tickets
    const long long tickets = ((long long)n_rays + NORMALS_TICKET_RAYS - 1) / NORMALS_TICKET_RAYS;
    long long grid = (long long)march_cu_count() * (cp ? 4 : 3);
    if (grid > (tickets + 3) / 4) grid = (tickets + 3) / 4;
    if (grid < 1) grid = 1;
    const float3 h3 = make_float3(h[0], h[1], h[2]), i3 = make_float3(inv2h[0], inv2h[1], inv2h[2]);
    const CpDev none = {};
    if (cp) hipLaunchKernelGGL((normals_kernel<true>), dim3((unsigned)grid), dim3(256), 0, stream, sc, *cp, mo, n_rays, h3, i3, normal_out, acc_out, depth_out);
    else hipLaunchKernelGGL((normals_kernel<false>), dim3((unsigned)grid), dim3(256), 0, stream, sc, none, mo, n_rays, h3, i3, normal_out, acc_out, depth_out);
    return hipGetLastError();
}
