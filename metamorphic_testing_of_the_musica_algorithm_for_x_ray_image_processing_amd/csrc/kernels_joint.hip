// kernels_joint.hip — the joint gray-level histogram of the study's tone metrics (musica_sim_joint, include/musica.h; harness.py
// joint_histogram) and the remap of a reference slot through a 256-entry table (musica_sim_remap_reference).
//
// k_joint: J[a][b] of a query = how many region pixels have the value a on side a (the graded f32 plane quantised with out_u8 while it
// is read: exactly what k_sim compares) and b on side b (a reference slot's u8 plane). Every query owns blockIdx.z, as in k_sim.
//   * The table is 256 x 256 counters. As u32 that is 256 KiB, which no workgroup can hold; as u16 it is 128 KiB, and a workgroup of
//     gfx950 may declare up to 160 KiB of LDS. So a workgroup of 1024 threads privatises the whole table as 32768 dwords of packed u16
//     pairs: bin = a * 256 + b lives in half (bin & 1) of dword bin >> 1 and is incremented with one LDS add of 1 << 16 * (bin & 1).
//     One workgroup per CU (LDS-limited), 16 wavefronts.
//   * The flush rule: a workgroup counts chunks of whole region rows, at most 65535 pixels each (at most kJointChunkPixels / w rows; w <= 16364),
//     and after every chunk adds its non-zero halves to the query's global u32 table with integer atomics and clears them. Between two
//     flushes a half receives at most 65535 increments, so it cannot wrap and nothing carries into its neighbour, even when every pixel
//     of the chunk falls into one bin (a flat image against a flat slot).
//   * Each region pixel is counted exactly once: chunks partition the rows, the threads of a workgroup partition a chunk's pixels.
//     All additions are integer, so the table is exact and identical from call to call whatever the order.
//   * Loads: a thread takes 4 consecutive pixels of a row, 16 B of side a and 4 B of side b. A region starts anywhere and the slot's
//     pitch N - 20 is rarely a multiple of 4, so neither load is naturally aligned: both are spelled as byte copies from pointers of
//     known lesser alignment, which gfx950's unaligned access mode turns into one global_load_dwordx4 and one global_load_dword. The
//     w % 4 pixels at the end of a row are read one at a time.
// MUSICA_JOINT_GLOBAL_ATOMICS (a devtools/build_variant.sh build, for the A/B of DESIGN.md section 4; not shipped) replaces the LDS
// table with one global atomic per pixel.
//
// k_sim_remap: dst[i] = lut[src[i]] over a dense plane, 8 pixels per thread as k_sim_vendor (8 B in, 8 B out, aligned from the
// allocations' bases), the table in LDS.
#include <algorithm>

#include "study_device.h"

namespace musica {

constexpr int kJointThreads = 1024;
constexpr int kJointDwords = 32768;          // 65536 u16 counters
constexpr int kJointChunkPixels = 65535;     // what a u16 half can count
constexpr int kJointQuads = 4;               // 4-pixel groups a thread loads before it counts them

__device__ __forceinline__ void joint_count(uint32_t* tab, uint32_t* __restrict__ out, uint32_t a, uint32_t b) {
    const uint32_t bin = (a << 8) | b;
#ifdef MUSICA_JOINT_GLOBAL_ATOMICS
    atomicAdd(&out[bin], 1u);
#else
    atomicAdd(&tab[bin >> 1], 1u << (16 * (bin & 1u)));
#endif
}

__global__ __launch_bounds__(kJointThreads) void k_joint(const JointQueryDev* __restrict__ qs, uint32_t* __restrict__ joint) {
#ifdef MUSICA_JOINT_GLOBAL_ATOMICS
    uint32_t* tab = nullptr;
#else
    __shared__ uint32_t tab[kJointDwords];
#endif
    const JointQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.chunks) return;   // whole workgroup: the grid is sized for the query with the most chunks
    const int t = threadIdx.x;
    uint32_t* __restrict__ out = joint + (size_t)blockIdx.z * 65536;
#ifndef MUSICA_JOINT_GLOBAL_ATOMICS
    for (int i = t; i < kJointDwords / 4; i += kJointThreads) reinterpret_cast<uint4*>(tab)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
#endif
    const int quads = q.w >> 2, tail = q.w & 3;
    for (int chunk = blockIdx.x; chunk < q.chunks; chunk += gridDim.x) {
        const int r0 = chunk * q.chunk_rows;
        const int rows = min(q.chunk_rows, q.h - r0);
        // the planes are device memory: say so, or the pointers read from the query are generic and the loads come out as flat_load
        const GlobalF32* __restrict__ pa = (const GlobalF32*)q.a + (size_t)r0 * q.a_pitch;
        const GlobalU8* __restrict__ pb = (const GlobalU8*)q.b + (size_t)r0 * q.b_pitch;
        const int items = rows * quads;
        for (int i0 = t; i0 < items; i0 += kJointQuads * kJointThreads) {
            float va[kJointQuads][4];
            uint32_t vb[kJointQuads];
#pragma unroll
            for (int u = 0; u < kJointQuads; u++) {   // all loads of the group first: 80 B in flight per thread
                const int i = min(i0 + u * kJointThreads, items - 1);   // past the end: the last quad again, not counted below
                const int r = i / quads, c = (i - r * quads) << 2;
                __builtin_memcpy(va[u], pa + (size_t)r * q.a_pitch + c, 16);   // 4-byte aligned
                __builtin_memcpy(&vb[u], pb + (size_t)r * q.b_pitch + c, 4);   // 1-byte aligned
            }
#pragma unroll
            for (int u = 0; u < kJointQuads; u++) {
                if (i0 + u * kJointThreads >= items) break;
#pragma unroll
                for (int k = 0; k < 4; k++) joint_count(tab, out, out_u8(va[u][k]), (vb[u] >> (8 * k)) & 0xFFu);
            }
        }
        for (int i = t; i < rows * tail; i += kJointThreads) {
            const int r = i / tail, c = (quads << 2) + (i - r * tail);
            joint_count(tab, out, out_u8(pa[(size_t)r * q.a_pitch + c]), pb[(size_t)r * q.b_pitch + c]);
        }
#ifndef MUSICA_JOINT_GLOBAL_ATOMICS
        __syncthreads();
        for (int i = t; i < kJointDwords / 4; i += kJointThreads) {
            const uint4 v = reinterpret_cast<uint4*>(tab)[i];
            if ((v.x | v.y | v.z | v.w) == 0u) continue;
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (d[k] & 0xFFFFu) atomicAdd(&out[8 * i + 2 * k], d[k] & 0xFFFFu);
                if (d[k] >> 16) atomicAdd(&out[8 * i + 2 * k + 1], d[k] >> 16);
            }
            reinterpret_cast<uint4*>(tab)[i] = make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
#endif
    }
}

// Workgroups a query of a launch of `count` gets: one round of the chip's 256 CUs over all queries (a CU holds one of these workgroups,
// and each pays for clearing and scanning its table), but at least kJointMinBlocks.
static int joint_blocks(int count) { return std::max(kJointMinBlocks, kJointMaxBlocks / count); }

void joint_geometry(JointQueryDev& q, int count) {
    // rows per chunk: what the u16 halves allow, less where the region would otherwise leave workgroups without a chunk
    const int blocks = joint_blocks(count);
    q.chunk_rows = std::max(1, std::min(kJointChunkPixels / q.w, (q.h + blocks - 1) / blocks));
    q.chunks = (q.h + q.chunk_rows - 1) / q.chunk_rows;
}

void launch_joint(hipStream_t st, const JointQueryDev* d_qs, int count, int max_chunks, uint32_t* joint) {
    // one workgroup per chunk up to joint_blocks; beyond that a workgroup strides over its query's chunks
    hipLaunchKernelGGL(k_joint, dim3(std::min(max_chunks, joint_blocks(count)), 1, count), dim3(kJointThreads), 0, st, d_qs, joint);
}

constexpr int kRemapThreads = 256;
constexpr int kRemapPx = 8;

__device__ __forceinline__ uint32_t remap4(const uint8_t* lut, uint32_t v) {
    return (uint32_t)lut[v & 0xFFu] | ((uint32_t)lut[(v >> 8) & 0xFFu] << 8) | ((uint32_t)lut[(v >> 16) & 0xFFu] << 16) | ((uint32_t)lut[v >> 24] << 24);
}

__global__ __launch_bounds__(kRemapThreads) void k_sim_remap(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, RemapLut lut, long long total) {
    __shared__ uint8_t sh[256];
    sh[threadIdx.x] = lut.v[threadIdx.x];
    __syncthreads();
    const long long p0 = ((long long)blockIdx.x * kRemapThreads + threadIdx.x) * kRemapPx;
    if (p0 >= total) return;
    if (p0 + kRemapPx > total) {
        for (long long p = p0; p < total; p++) out[p] = sh[src[p]];
        return;
    }
    const uint2 v = *reinterpret_cast<const uint2*>(src + p0);
    *reinterpret_cast<uint2*>(out + p0) = make_uint2(remap4(sh, v.x), remap4(sh, v.y));
}

void launch_sim_remap(hipStream_t st, const uint8_t* src, uint8_t* out, const RemapLut& lut, long long total) {
    const long long threads = (total + kRemapPx - 1) / kRemapPx;
    const unsigned blocks = (unsigned)((threads + kRemapThreads - 1) / kRemapThreads);
    hipLaunchKernelGGL(k_sim_remap, dim3(blocks), dim3(kRemapThreads), 0, st, src, out, lut, total);
}

}  // namespace musica
