// kernels_export.hip — the 8-bit output of a range of batch images into caller-owned device memory (musica_export_out, gfx950).
//
//   k_export_u8 : saveOutImage's crop + quantise (k_out_pixels' statement: out_u8, kernels_common.h) for `count` images in ONE
//                 launch (blockIdx.z = image, as k_grad_apply), written through the caller's row and image pitches. Each lane turns 16
//                 consecutive output pixels of one row into 16 bytes: the source run starts MUSICA_OUT_MARGIN = 10 floats into a row whose
//                 start is 16-byte aligned (pitch is a multiple of 4 floats), i.e. on an 8-byte boundary, so it is read as eight 8-byte
//                 loads; the 16 bytes leave as one 16-byte store when the destination, its row pitch and its image pitch allow it (W), else
//                 as 8-, 4- or 1-byte pieces. The last lane of a row (N - 20 is rarely a multiple of 16) reads and writes only its own pixels.
#include <stdint.h>
#include "kernels_common.h"
#include "launchers.h"

namespace musica {

static_assert((MUSICA_OUT_MARGIN & 1) == 0, "k_export_u8 reads the cropped rows as 8-byte pairs: the margin must be even");

template <int W>   // bytes per store: 16, 8, 4 or 1
__global__ __launch_bounds__(256) void k_export_u8(const float* __restrict__ graded, int pitch, size_t plane, int nw, int lanes_per_row,
                                                   uint8_t* __restrict__ dst, size_t row_pitch, size_t image_pitch) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = idx / lanes_per_row;
    if (y >= nw) return;
    const int x0 = (idx - y * lanes_per_row) * 16;
    const float* src = graded + (size_t)blockIdx.z * plane + (size_t)(y + MUSICA_OUT_MARGIN) * pitch + MUSICA_OUT_MARGIN + x0;
    uint8_t* out = dst + (size_t)blockIdx.z * image_pitch + (size_t)y * row_pitch + x0;
    if (x0 + 16 > nw) {   // ragged tail of the row
        for (int j = 0; x0 + j < nw; j++) out[j] = (uint8_t)out_u8(src[j]);
        return;
    }
    const float2* s2 = reinterpret_cast<const float2*>(src);
    float2 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = s2[k];
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
        w[k] = out_u8(v[2 * k].x) | (out_u8(v[2 * k].y) << 8) | (out_u8(v[2 * k + 1].x) << 16) | (out_u8(v[2 * k + 1].y) << 24);
    if constexpr (W == 16) {
        *reinterpret_cast<uint4*>(out) = make_uint4(w[0], w[1], w[2], w[3]);
    } else if constexpr (W == 8) {
        reinterpret_cast<uint2*>(out)[0] = make_uint2(w[0], w[1]);
        reinterpret_cast<uint2*>(out)[1] = make_uint2(w[2], w[3]);
    } else if constexpr (W == 4) {
#pragma unroll
        for (int k = 0; k < 4; k++) reinterpret_cast<uint32_t*>(out)[k] = w[k];
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) out[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

void launch_export_u8(hipStream_t st, const float* graded, const LevelDesc& l0, int count, uint8_t* dst, size_t row_pitch, size_t image_pitch) {
    const int nw = l0.S - 2 * MUSICA_OUT_MARGIN;
    const int lanes_per_row = (nw + 15) / 16;
    const dim3 grid((unsigned)(((size_t)nw * lanes_per_row + 255) / 256), 1, (unsigned)count);
    // the widest store every row start allows: the destination, its row pitch and (with more than one image) its image pitch
    const uintptr_t bits = (uintptr_t)dst | (uintptr_t)row_pitch | (count > 1 ? (uintptr_t)image_pitch : 0);
    auto* kern = (bits & 15) == 0 ? k_export_u8<16> : (bits & 7) == 0 ? k_export_u8<8> : (bits & 3) == 0 ? k_export_u8<4> : k_export_u8<1>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, graded, l0.pitch, l0.plane, nw, lanes_per_row, dst, row_pitch, image_pitch);
}

}  // namespace musica
