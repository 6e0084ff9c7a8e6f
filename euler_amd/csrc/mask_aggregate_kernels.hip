// Layerwise-adjacency aggregation straight from the bit mask (GCNAggregator / MeanAggregator of
// tf_euler/python/utils/sparse_aggregators.py:37-84) on the matrix units of gfx950, the 64 x 64
// bit-block transpose its gradient needs, and their C-ABI entry points.  The contract, the tiling,
// the operand layouts and the LDS budget are stated in mp_mask.h; this file is the kernels and the
// dispatch ladder.
//
// THE KERNEL, per work item (batch row, source tile, column tile): per candidate block the lanes
// first fetch their sources' words of the block, then the workgroup stages the block's slice of x
// in LDS (16 bits: transposed in registers, 16-byte units; fp32: row-major), and every wave walks
// the words: one ballot per run for the zero-word skip, then per chunk of 32 candidates the mask
// byte expanded to an A fragment per run and, per column fragment, ONE B read shared by both runs.
// The epilogue adds the root, divides, narrows and stores from the accumulator layout.
// No atomics, no scratch, no host wait: one launch on the caller's stream.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_mask_frag.h"

namespace euler_gpu {
namespace {

struct MaskArgs {
  const uint64_t* mask;
  const void* x;
  const void* root;
  void* out;
  float* degree_out;
  int64_t batch;
  int32_t n, m, d, op, out_f32, words, waves;
  MaskPlan plan;
};

// words of a candidate block
template <int DT>
constexpr int MaskBlockWords() { return (DT == kF32 ? kMaskBlock32 : kMaskBlock16) / 64; }

// The block's slice of x into LDS.  Rows c0 + k < m of batch row b and columns f0 + f < d; +0 else
template <int DT, int NT, bool VEC>
__device__ __forceinline__ void MaskStage(const MaskArgs& a, int64_t row0, int32_t c0, int32_t f0, unsigned char* lds) {
  constexpr int kPieces = 2 * NT;                  // pieces of 8 columns in the column tile
  const int32_t stride = a.plan.stride;
  if constexpr (DT == kF32) {
    const int32_t total = a.plan.kb * kPieces;
    for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
      const int32_t fb = i % kPieces, k = i / kPieces;
      DenseWords r[2];
      DenseLoadA<DT, VEC>(a.x, c0 + k < a.m ? (row0 + c0 + k) * a.d : -1, f0 + 8 * fb, a.d, r);
      DenseWords* to = reinterpret_cast<DenseWords*>(lds + k * stride + fb * 32);
      to[0] = r[0];
      to[1] = r[1];
    }
  } else {
    const int32_t total = (a.plan.kb / 8) * kPieces;
    for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
      const int32_t fb = i % kPieces, kblk = i / kPieces;
      DenseWords r[8];                             // r[k][p]: columns 2 p, 2 p + 1 of candidate k
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int32_t c = c0 + 8 * kblk + k;
        DenseLoadA<DT, VEC>(a.x, c < a.m ? (row0 + c) * a.d : -1, f0 + 8 * fb, a.d, &r[k]);
      }
#pragma unroll
      for (int f = 0; f < 8; ++f) {                // column f of the block: candidates 2 q, 2 q + 1 per word
        DenseWords t;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t lo = r[2 * q][f / 2], hi = r[2 * q + 1][f / 2];
          t[q] = f % 2 == 0 ? (lo & 0xffffu) | (hi << 16) : (lo >> 16) | (hi & 0xffff0000u);
        }
        *reinterpret_cast<DenseWords*>(lds + MaskXtByte(8 * fb + f, 16 * kblk, stride)) = t;
      }
    }
  }
}

// The A fragment of lane group g for chunk x (0, 1) of a word.  16 bits: one byte -> eight ones or
// zeros; fp32: element j is candidate 4 j + g of the chunk
template <int DT>
__device__ __forceinline__ void MaskFragment(uint64_t word, int x, int32_t g, DenseWords* af) {
  const uint32_t half = (uint32_t)(word >> (32 * x));
  if constexpr (DT == kF32) {
    const uint32_t bits = half >> g;
#pragma unroll
    for (int j = 0; j < 8; ++j) af[j / 4][j % 4] = (bits >> (4 * j)) & 1u ? 0x3f800000u : 0u;
  } else {
    constexpr uint32_t kOne = DT == kBF16 ? 0x3f80u : 0x3c00u;
    const uint32_t byte = half >> (8 * g);
#pragma unroll
    for (int p = 0; p < 4; ++p)
      af[0][p] = ((byte >> (2 * p)) & 1u ? kOne : 0u) | ((byte >> (2 * p + 1)) & 1u ? kOne << 16 : 0u);
  }
}

extern __shared__ __align__(16) unsigned char mask_lds[];

template <int DT, int NT, bool VEC>
__global__ __launch_bounds__(64 * kMaskWaves, 2) void MaskAggregateKernel(const MaskArgs a) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int KW = MaskBlockWords<DT>();
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const int32_t tile = a.waves * kMaskRuns * kPoolTile;
  const int64_t tiles = ((int64_t)a.n + tile - 1) / tile;
  const int64_t items = a.batch * tiles * a.plan.col_tiles;
  const int32_t stride = a.plan.stride;
  const uint64_t tail = a.m % 64 ? (1ull << (a.m % 64)) - 1ull : ~0ull;   // the live bits of the last word

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int32_t ct = (int32_t)(item % a.plan.col_tiles);
    const int64_t b = item / a.plan.col_tiles / tiles;
    const int32_t s0 = (int32_t)(item / a.plan.col_tiles % tiles) * tile + wave * kMaskRuns * kPoolTile;
    const int32_t f0 = ct * 16 * NT;
    // this lane's source of each run: its mask row, or none
    const uint64_t* mrow[kMaskRuns];
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q) {
      const int32_t src = s0 + q * kPoolTile + c;
      mrow[q] = src < a.n ? a.mask + (b * a.n + src) * (int64_t)a.words : nullptr;
    }
    int32_t deg[kMaskRuns] = {0, 0};
    DenseAcc acc[kMaskRuns][NT];
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q)
#pragma unroll
      for (int nf = 0; nf < NT; ++nf) acc[q][nf] = DenseAcc{0.f, 0.f, 0.f, 0.f};

    for (int32_t c0 = 0; c0 < a.m; c0 += a.plan.kb) {
      const int32_t w0 = c0 / 64;
      const int32_t live = a.words - w0 < a.plan.kb / 64 ? a.words - w0 : a.plan.kb / 64;
      uint64_t word[kMaskRuns][KW];
#pragma unroll
      for (int q = 0; q < kMaskRuns; ++q)
#pragma unroll
        for (int w = 0; w < KW; ++w) {
          word[q][w] = (mrow[q] && w < live) ? mrow[q][w0 + w] : 0ull;
          if (w0 + w == a.words - 1) word[q][w] &= tail;
          deg[q] += __popcll(word[q][w]);
        }
      __syncthreads();                             // the previous block's B reads are done
      MaskStage<DT, NT, VEC>(a, b * a.m, c0, f0, mask_lds);
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
          DenseWords af[kMaskRuns][FW];
#pragma unroll
          for (int q = 0; q < kMaskRuns; ++q) MaskFragment<DT>(word[q][w], x, g, af[q]);
#pragma unroll
          for (int nf = 0; nf < NT; ++nf) {
            DenseWords bw[FW];
            MaskLoadB<DT>(mask_lds, stride, 64 * w + 32 * x, nf, c, g, bw);
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
      if (a.degree_out && ct == 0 && g == 0 && r0 + c < a.n) a.degree_out[b * a.n + r0 + c] = (float)deg[q];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float dg = (float)__shfl(deg[q], 4 * g + i);      // lane 4 g + i holds source 4 g + i of the run
        const int32_t src = r0 + 4 * g + i;
        if (src >= a.n) continue;
        const int64_t at = (b * a.n + src) * a.d;
#pragma unroll
        for (int nf = 0; nf < NT; ++nf) {
          const int32_t col = f0 + 16 * nf + c;
          if (col >= a.d) continue;
          // one division for the three dividing ops: the root goes in before it (renorm) or after it (gcn)
          const float root = a.root ? MaskRoot<DT>(a.root, at + col) : 0.f;
          float v = a.op == kMaskGcnRenorm ? MpwAdd(root, acc[q][nf][i]) : acc[q][nf][i];
          if (a.op != kMaskAdd) v = MpwDiv(v, a.op == kMaskGcnRenorm ? MaskRenormDenominator(dg) : MaskMeanDenominator(dg));
          if (a.op == kMaskGcn) v = MpwAdd(root, v);
          if (DT == kF32 || a.out_f32) static_cast<float*>(a.out)[at + col] = v;
          else if constexpr (DT != kF32) static_cast<uint16_t*>(a.out)[at + col] = HalfCvt<DT>::Narrow(v);
        }
      }
    }
  }
}

template <int DT, int NT, bool VEC>
int MaskLaunch(hipStream_t st, const MaskArgs& a) {
  const int64_t tile = MaskTile(a.waves);
  const int64_t items = a.batch * ((a.n + tile - 1) / tile) * a.plan.col_tiles;
  const unsigned blocks = (unsigned)(items > kMaskMaxBlocks ? kMaskMaxBlocks : items);
  hipLaunchKernelGGL((MaskAggregateKernel<DT, NT, VEC>), dim3(blocks), dim3(64 * a.waves), (size_t)a.plan.lds_bytes, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT, int NT>
int MaskDispatchLoads(hipStream_t st, const MaskArgs& a) {
  return PoolVectorLoads(a.d, (uintptr_t)a.x, DT == kF32) ? MaskLaunch<DT, NT, true>(st, a) : MaskLaunch<DT, NT, false>(st, a);
}

template <int DT>
int MaskDispatchTile(hipStream_t st, const MaskArgs& a) {
  switch (a.plan.nt) {
    case 1: return MaskDispatchLoads<DT, 1>(st, a);
    case 2: return MaskDispatchLoads<DT, 2>(st, a);
    case 4: return MaskDispatchLoads<DT, 4>(st, a);
    default: return MaskDispatchLoads<DT, 8>(st, a);
  }
}

// One wave per 64 x 64 bit block: lane l reads word jb of source 64 ib + l and leaves with word ib
// of candidate 64 jb + l - bit k of every lane gathered by one ballot per k.
constexpr int kTransposeWaves = 4;
constexpr int kTransposeMaxBlocks = 4096;

__global__ __launch_bounds__(64 * kTransposeWaves) void MaskTransposeKernel(const uint64_t* mask, int64_t batch, int32_t n,
                                                                            int32_t m, uint64_t* out) {
  const int32_t lane = threadIdx.x & 63;
  const int32_t words_m = (m + 63) / 64, words_n = (n + 63) / 64;
  const int64_t blocks = batch * words_n * words_m;
  const uint64_t tail = m % 64 ? (1ull << (m % 64)) - 1ull : ~0ull;
  for (int64_t blk = (int64_t)blockIdx.x * kTransposeWaves + (threadIdx.x >> 6); blk < blocks;
       blk += (int64_t)gridDim.x * kTransposeWaves) {
    const int32_t jb = (int32_t)(blk % words_m), ib = (int32_t)(blk / words_m % words_n);
    const int64_t b = blk / words_m / words_n;
    const int32_t src = 64 * ib + lane;
    uint64_t word = src < n ? mask[(b * n + src) * words_m + jb] : 0ull;
    if (jb == words_m - 1) word &= tail;
    uint64_t res = 0ull;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) {
      const uint64_t column = __builtin_amdgcn_ballot_w64((word >> k) & 1ull);
      if (lane == k) res = column;
    }
    const int32_t cand = 64 * jb + lane;
    if (cand < m) out[(b * m + cand) * words_n + ib] = res;
  }
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

namespace { constexpr int64_t kBig = 1LL << 31; }

extern "C" {

int euler_gpu_mask_aggregate(void* stream, int32_t op, const uint64_t* mask_dev, const void* x_dev, int32_t dtype,
                             int64_t x_rows, const void* root_dev, int64_t batch, int64_t n, int64_t m, int64_t d,
                             void* out_dev, int32_t out_dtype, float* degree_out_dev) {
  const std::string what("mask_aggregate");
  if (op < kMaskAdd || op > kMaskGcnRenorm)
    return Fail(EULER_GPU_EINVAL, what + ": op is 0 add, 1 mean, 2 gcn, 3 gcn_renorm");
  if (!KnownDtype(dtype) || !KnownDtype(out_dtype)) return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != dtype) return Fail(EULER_GPU_EINVAL, what + ": out is fp32 or of x's dtype");
  if (batch < 0 || n < 0 || m < 0) return Fail(EULER_GPU_EINVAL, what + ": batch, n or m < 0");
  if (batch >= kBig || n >= kBig || m >= kBig || batch * n >= kBig || batch * m >= kBig)
    return Fail(EULER_GPU_EINVAL, what + ": batch * n or batch * m >= 2^31");
  if (d < 1 || d > kMaskMaxD) return Fail(EULER_GPU_EINVAL, what + ": d outside 1..1024");
  if (x_rows < batch * m) return Fail(EULER_GPU_EINVAL, what + ": x has fewer than batch * m rows");
  if (batch * n == 0) return EULER_GPU_OK;
  const bool gcn = op == kMaskGcn || op == kMaskGcnRenorm;
  if ((m > 0 && (!mask_dev || !x_dev)) || !out_dev || (gcn && !root_dev)) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  const uintptr_t esz = dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)mask_dev % 8 != 0 || (uintptr_t)x_dev % esz != 0 || (uintptr_t)root_dev % esz != 0 ||
      (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 4 : 2) != 0 || (uintptr_t)degree_out_dev % 4 != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  MaskArgs a{};
  a.mask = mask_dev; a.x = x_dev; a.root = gcn ? root_dev : nullptr; a.out = out_dev; a.degree_out = degree_out_dev;
  a.batch = batch; a.n = (int32_t)n; a.m = (int32_t)m; a.d = (int32_t)d; a.op = op;
  a.out_f32 = out_dtype == EULER_GPU_F32; a.words = (int32_t)((m + 63) / 64);
  a.plan = MaskMakePlan(m, d, dtype == EULER_GPU_F32);
  a.waves = MaskWaves(batch, n, a.plan.col_tiles);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EULER_GPU_F32) return MaskDispatchTile<kF32>(st, a);
  if (dtype == EULER_GPU_BF16) return MaskDispatchTile<kBF16>(st, a);
  return MaskDispatchTile<kF16>(st, a);
}

int euler_gpu_mask_transpose(void* stream, const uint64_t* mask_dev, int64_t batch, int64_t n, int64_t m,
                             uint64_t* out_dev) {
  const std::string what("mask_transpose");
  if (batch < 0 || n < 0 || m < 0) return Fail(EULER_GPU_EINVAL, what + ": batch, n or m < 0");
  if (batch >= kBig || n >= kBig || m >= kBig || batch * n >= kBig || batch * m >= kBig)
    return Fail(EULER_GPU_EINVAL, what + ": batch * n or batch * m >= 2^31");
  if (batch * n == 0 || m == 0) return EULER_GPU_OK;
  if (!mask_dev || !out_dev) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if ((uintptr_t)mask_dev % 8 != 0 || (uintptr_t)out_dev % 8 != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  const int64_t blocks = batch * ((n + 63) / 64) * ((m + 63) / 64);
  const int64_t groups = (blocks + kTransposeWaves - 1) / kTransposeWaves;
  hipLaunchKernelGGL(MaskTransposeKernel, dim3((unsigned)(groups > kTransposeMaxBlocks ? kTransposeMaxBlocks : groups)),
                     dim3(64 * kTransposeWaves), 0, (hipStream_t)stream, mask_dev, batch, (int32_t)n, (int32_t)m, out_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // extern "C"
