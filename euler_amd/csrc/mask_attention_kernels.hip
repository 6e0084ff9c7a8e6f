// Layerwise attention aggregation straight from the bit mask (AttentionAggregator of
// tf_euler/python/utils/sparse_aggregators.py:87-139) on the matrix units of gfx950, and its C-ABI entry
// point.  The contract, the arithmetic, the tiling and the LDS budget are stated in mp_mask_attention.h;
// this file is the kernel and the dispatch ladder.
//
// THE KERNEL, per work item (batch row, source tile, head, column tile of the head): pass 1 walks the
// sources' mask words over the head's staged s_nb blocks for the per-source maximum; pass 2 stages per
// candidate block the head's slice of z (16 bits: transposed in registers, 16-byte units; fp32:
// row-major) and the scores again, and per chunk of 32 candidates every lane builds its A fragment of
// eight softmax numerators in registers, adds them to its partial denominator and multiplies; ONE B
// read is shared by both runs of the wave.  The epilogue adds the self term, divides, adds the root,
// applies relu, narrows and stores from the accumulator layout.
// No atomics, no scratch, no host wait: one launch on the caller's stream.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_mask_attention.h"
#include "mp_mask_attention_frag.h"

namespace euler_gpu {
namespace {

// The A fragment of one run for a chunk: the eight numerators, rounded once to the operand type, and
// the same rounded values added to the lane's partial denominator in increasing c
template <int DT>
__device__ __forceinline__ void AttFragment(uint32_t half, int32_t g, const float* s, float s_src, float shift, float slope,
                                            DenseWords* af, float* l) {
  float p[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float pv = AttExp(AttAdditiveLogit(s_src, s[j], slope), shift);
    p[j] = AttBit<DT>(half, g, j) ? pv : 0.f;
  }
  if constexpr (DT == kF32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      af[j / 4][j % 4] = F32Bits(p[j]);
      *l = MpwAdd(*l, p[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t w = Narrow2<DT>(p[2 * j], p[2 * j + 1]);
      float lo, hi;
      Widen2<DT>(w, &lo, &hi);
      af[0][j] = w;
      *l = MpwAdd(MpwAdd(*l, lo), hi);
    }
  }
}

extern __shared__ __align__(16) unsigned char mask_att_lds[];

template <int DT, int NT, bool VEC>
__global__ __launch_bounds__(64 * kMaskWaves, 2) void MaskAttentionKernel(const MaskAttArgs a) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int KW = AttBlockWords<DT>();
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const int32_t tile = a.waves * kMaskRuns * kPoolTile;
  const int64_t tiles = ((int64_t)a.n + tile - 1) / tile;
  const int32_t head_items = a.heads * a.plan.col_tiles;
  const int64_t items = a.batch * tiles * head_items;
  const int32_t stride = a.plan.stride;
  const uint64_t tail = a.m % 64 ? (1ull << (a.m % 64)) - 1ull : ~0ull;   // the live bits of the last word
  float* sc = reinterpret_cast<float*>(mask_att_lds + a.plan.score_off);

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int32_t ct = (int32_t)(item % a.plan.col_tiles);
    const int32_t h = (int32_t)(item / a.plan.col_tiles % a.heads);
    const int64_t b = item / head_items / tiles;
    const int32_t s0 = (int32_t)(item / head_items % tiles) * tile + wave * kMaskRuns * kPoolTile;
    const int32_t f0 = ct * 16 * NT, col0 = h * a.dh;
    // this lane's source of each run: its mask row and its scores, or none
    const uint64_t* mrow[kMaskRuns];
    float s_src[kMaskRuns], e0[kMaskRuns], mx[kMaskRuns], l[kMaskRuns] = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q) {
      const int32_t src = s0 + q * kPoolTile + c;
      const bool on = src < a.n;
      mrow[q] = on ? a.mask + (b * a.n + src) * (int64_t)a.words : nullptr;
      s_src[q] = on ? a.s_src[(b * a.n + src) * a.heads + h] : 0.f;
      e0[q] = a.s_root ? AttAdditiveLogit(s_src[q], on ? a.s_root[(b * a.n + src) * a.heads + h] : 0.f, a.slope) : 0.f;
      mx[q] = -__builtin_inff();
    }

    // pass 1: the largest neighbour score of every source
    for (int64_t c64 = 0; c64 < a.m; c64 += a.plan.kb) {      // (64 bits: m + kb may pass 2^31)
      const int32_t c0 = (int32_t)c64, w0 = c0 / 64;
      const int32_t live = a.words - w0 < a.plan.kb / 64 ? a.words - w0 : a.plan.kb / 64;
      uint64_t word[kMaskRuns][KW];
      AttLoadWords<KW>(mrow, w0, live, a.words, tail, word);
      __syncthreads();                             // the previous block's score reads are done
      AttStageScores(a, b * a.m, h, c0, sc);
      __syncthreads();
#pragma unroll
      for (int w = 0; w < KW; ++w) {
        if (w >= live) break;
#pragma unroll
        for (int x = 0; x < 2; ++x) {
          float s[8];
          AttScores<DT>(sc, 64 * w + 32 * x, g, s);
#pragma unroll
          for (int q = 0; q < kMaskRuns; ++q) {
            const uint32_t half = (uint32_t)(word[q][w] >> (32 * x));
#pragma unroll
            for (int j = 0; j < 8; ++j) mx[q] = (AttBit<DT>(half, g, j) && s[j] > mx[q]) ? s[j] : mx[q];
          }
        }
      }
    }
    // the four lane groups of a source, then the shift: leaky is monotone, so the leaky of the
    // largest score is the largest logit
    float shift[kMaskRuns];
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q) {
      float v = mx[q];
      const float v16 = __shfl_xor(v, 16);
      v = v16 > v ? v16 : v;
      const float v32 = __shfl_xor(v, 32);
      v = v32 > v ? v32 : v;
      // (no neighbour: the shift stays -inf, never leaky(-inf) - that is NaN at slope 0 - and every p is selected to +0)
      shift[q] = v > -__builtin_inff() ? AttAdditiveLogit(s_src[q], v, a.slope) : v;
      if (a.s_root) shift[q] = e0[q] > shift[q] ? e0[q] : shift[q];
    }

    DenseAcc acc[kMaskRuns][NT];
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q)
#pragma unroll
      for (int nf = 0; nf < NT; ++nf) acc[q][nf] = DenseAcc{0.f, 0.f, 0.f, 0.f};

    // pass 2: numerators in registers, denominators beside them, products on the matrix units
    for (int64_t c64 = 0; c64 < a.m; c64 += a.plan.kb) {      // (64 bits: m + kb may pass 2^31)
      const int32_t c0 = (int32_t)c64, w0 = c0 / 64;
      const int32_t live = a.words - w0 < a.plan.kb / 64 ? a.words - w0 : a.plan.kb / 64;
      uint64_t word[kMaskRuns][KW];
      AttLoadWords<KW>(mrow, w0, live, a.words, tail, word);
      __syncthreads();                             // the previous block's reads (pass 1's too) are done
      AttStage<DT, NT, VEC>(a, b * a.m, col0, c0, f0, mask_att_lds);
      AttStageScores(a, b * a.m, h, c0, sc);
      __syncthreads();
#pragma unroll
      for (int w = 0; w < KW; ++w) {
        if (w >= live) break;
        bool any[kMaskRuns];
#pragma unroll
        for (int q = 0; q < kMaskRuns; ++q) any[q] = __builtin_amdgcn_ballot_w64(word[q][w] != 0ull) != 0ull;
        if (!any[0] && !any[1]) continue;
#pragma unroll
        for (int x = 0; x < 2; ++x) {
          float s[8];
          AttScores<DT>(sc, 64 * w + 32 * x, g, s);
          DenseWords af[kMaskRuns][FW];
#pragma unroll
          for (int q = 0; q < kMaskRuns; ++q)
            if (any[q])
              AttFragment<DT>((uint32_t)(word[q][w] >> (32 * x)), g, s, s_src[q], shift[q], a.slope, af[q], &l[q]);
#pragma unroll
          for (int nf = 0; nf < NT; ++nf) {
            DenseWords bw[FW];
            MaskLoadB<DT>(mask_att_lds, stride, 64 * w + 32 * x, nf, c, g, bw);
#pragma unroll
            for (int q = 0; q < kMaskRuns; ++q)
              if (any[q]) acc[q][nf] = DenseMma<DT>(af[q], bw, acc[q][nf]);
          }
        }
      }
    }

    // the epilogue, in the accumulator layout: rows 4 g + i of column c of every fragment
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q) {
      const int32_t r0 = s0 + q * kPoolTile;
      // the denominator of source c: the four lane groups in order, then the self term
      float lt = MpwAdd(MpwAdd(MpwAdd(__shfl(l[q], c), __shfl(l[q], c + 16)), __shfl(l[q], c + 32)), __shfl(l[q], c + 48));
      float p0 = 0.f;
      if (a.s_root) {
        p0 = AttExp(e0[q], shift[q]);
        lt = MpwAdd(lt, p0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float den = MaskAttDenominator(__shfl(lt, 4 * g + i));      // lane 4 g + i holds source 4 g + i of the run
        const float self = __shfl(p0, 4 * g + i);
        const int32_t src = r0 + 4 * g + i;
        if (src >= a.n) continue;
        const int64_t at = (b * a.n + src) * a.d + col0;
#pragma unroll
        for (int nf = 0; nf < NT; ++nf) {
          const int32_t col = f0 + 16 * nf + c;
          if (col >= a.dh) continue;
          const float root = a.root ? MaskRoot<DT>(a.root, at + col) : 0.f;
          float v = acc[q][nf][i];
          if (a.s_root) v = MpwAdd(v, MpwMul(self, root));
          v = MpwDiv(v, den);
          if (a.root && !a.s_root) v = MpwAdd(root, v);
          if (a.relu) v = v <= 0.f ? 0.f : v;
          if (DT == kF32 || a.out_f32) static_cast<float*>(a.out)[at + col] = v;
          else if constexpr (DT != kF32) static_cast<uint16_t*>(a.out)[at + col] = HalfCvt<DT>::Narrow(v);
        }
      }
    }
  }
}

template <int DT, int NT, bool VEC>
int AttLaunch(hipStream_t st, const MaskAttArgs& a) {
  const int64_t tile = MaskTile(a.waves);
  const int64_t items = a.batch * ((a.n + tile - 1) / tile) * a.heads * a.plan.col_tiles;
  const unsigned blocks = (unsigned)(items > kMaskMaxBlocks ? kMaskMaxBlocks : items);
  hipLaunchKernelGGL((MaskAttentionKernel<DT, NT, VEC>), dim3(blocks), dim3(64 * a.waves), (size_t)a.plan.lds_bytes, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT, int NT>
int AttDispatchLoads(hipStream_t st, const MaskAttArgs& a) {
  return PoolVectorLoads(a.dh, (uintptr_t)a.z, DT == kF32) ? AttLaunch<DT, NT, true>(st, a) : AttLaunch<DT, NT, false>(st, a);
}

template <int DT>
int AttDispatchTile(hipStream_t st, const MaskAttArgs& a) {
  switch (a.plan.nt) {
    case 1: return AttDispatchLoads<DT, 1>(st, a);
    case 2: return AttDispatchLoads<DT, 2>(st, a);
    default: return AttDispatchLoads<DT, 4>(st, a);
  }
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" int euler_gpu_mask_attention(void* stream, const uint64_t* mask_dev, const void* z_dev, int32_t dtype,
                                        int64_t z_rows, const float* s_src_dev, const float* s_nb_dev, int64_t s_nb_rows,
                                        const void* root_dev, const float* s_root_dev, int64_t batch, int64_t n, int64_t m,
                                        int64_t d, int64_t heads, float negative_slope, int32_t activation, void* out_dev,
                                        int32_t out_dtype) {
  constexpr int64_t kBig = 1LL << 31;
  const std::string what("mask_attention");
  if (!KnownDtype(dtype) || !KnownDtype(out_dtype)) return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != dtype) return Fail(EULER_GPU_EINVAL, what + ": out is fp32 or of z's dtype");
  if (activation != kMaskAttNone && activation != kMaskAttRelu) return Fail(EULER_GPU_EINVAL, what + ": activation is 0 none, 1 relu");
  if (!(negative_slope >= 0.f) || negative_slope > 3.0e38f)
    return Fail(EULER_GPU_EINVAL, what + ": negative_slope is finite and >= 0");
  if (batch < 0 || n < 0 || m < 0) return Fail(EULER_GPU_EINVAL, what + ": batch, n or m < 0");
  if (batch >= kBig || n >= kBig || m >= kBig || batch * n >= kBig || batch * m >= kBig)
    return Fail(EULER_GPU_EINVAL, what + ": batch * n or batch * m >= 2^31");
  if (d < 1 || d > kMaskMaxD) return Fail(EULER_GPU_EINVAL, what + ": d outside 1..1024");
  if (heads < 1 || d % heads != 0) return Fail(EULER_GPU_EINVAL, what + ": heads >= 1 divides d");
  if (z_rows < batch * m || s_nb_rows < batch * m) return Fail(EULER_GPU_EINVAL, what + ": z or s_nb has fewer than batch * m rows");
  if (s_root_dev && !root_dev) return Fail(EULER_GPU_EINVAL, what + ": s_root goes with root only");
  if (batch * n == 0) return EULER_GPU_OK;
  if ((m > 0 && (!mask_dev || !z_dev || !s_nb_dev)) || !s_src_dev || !out_dev) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  const uintptr_t esz = dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)mask_dev % 8 != 0 || (uintptr_t)z_dev % esz != 0 || (uintptr_t)root_dev % esz != 0 ||
      (uintptr_t)s_src_dev % 4 != 0 || (uintptr_t)s_nb_dev % 4 != 0 || (uintptr_t)s_root_dev % 4 != 0 ||
      (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 4 : 2) != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  MaskAttArgs a{};
  a.mask = mask_dev; a.z = z_dev; a.s_src = s_src_dev; a.s_nb = s_nb_dev; a.root = root_dev; a.s_root = s_root_dev;
  a.out = out_dev; a.batch = batch; a.n = (int32_t)n; a.m = (int32_t)m; a.d = (int32_t)d; a.heads = (int32_t)heads;
  a.dh = (int32_t)(d / heads); a.relu = activation == kMaskAttRelu; a.out_f32 = out_dtype == EULER_GPU_F32;
  a.words = (int32_t)((m + 63) / 64); a.slope = negative_slope;
  a.plan = MaskAttMakePlan(m, a.dh, dtype == EULER_GPU_F32);
  a.waves = MaskWaves(batch, n, a.heads * a.plan.col_tiles);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EULER_GPU_F32) return AttDispatchTile<kF32>(st, a);
  if (dtype == EULER_GPU_BF16) return AttDispatchTile<kBF16>(st, a);
  return AttDispatchTile<kF16>(st, a);
}
