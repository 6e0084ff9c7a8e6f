// Fused mean-aggregator layer over a quantised row table (Fp8Rows) on the matrix units of gfx950,
// with its C-ABI entry point: aggregate_dense (mp_dense.h) whose gathered rows - and, by index, whose
// root rows - are e4m3fn codes with one fp32 scale per column.  The contract, the block layout and
// the permutation of W^T in LDS are stated in mp_dense_fp8.h; this file is the kernel and its
// dispatch ladder.
//
// THE KERNEL is aggregate_dense_kernels.hip's, with another way into the fold.  Per F-tile pass the
// workgroup stages W^T through Fp8DenseRow (an indexed root's root_weight too; a dense root's as it
// is), then every wave takes runs of 16 destinations.  Per fold tile of 128 k = 2 blocks of 64
// codes: lane l holds the sixteen column scales of each block (32 registers), walks its positions
// in batches - the indices of a batch, then all its 16-byte loads, 2 per position, then decode,
// multiply and add in increasing p - into 32 fp32 registers, divides for mean, narrows, and feeds
// the registers to the MFMAs: values 0..7 of block b are the A fragment of chunk 2 b, values 8..15
// of chunk 2 b + 1.  An indexed root row is loaded the same way, once per fold tile, and either
// seeds the fold or is narrowed into the self path's A fragments; a dense root goes the old way.
// The root kind is a runtime flag.  No staging LDS, no atomics, no scratch, no host wait: one launch
// on the caller's stream.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_dense_fp8.h"
#include "mp_dense_frag.h"
#include "mp_fp8.h"

namespace euler_gpu {
namespace {

struct Fp8DenseArgs {
  const uint8_t* q; const float* scale; int64_t rows;
  const void* weight;
  const void* bias; int32_t bias_f32;
  const void* gather; int32_t is_ids;
  const int64_t* seg_ptr; int64_t count, e;
  const void* root;                                  // a dense root [size, ds], or
  const void* root_index; int32_t root_is_ids;       // rows of the table, [size]
  const void* root_weight;
  float root_scale; int32_t has_scale;
  int32_t d, ds, f, fs, size, op, act, combine;
  void* out; int32_t out_f32;
  DensePlan plan;
};

constexpr int kFp8DenseBlocks = kDenseFoldTile / kFp8DenseBlock;      // blocks of a fold tile

// positions whose loads are issued together: 8 x 2 x 16 bytes = 64 registers of codes in flight; at
// NT = 8, where two accumulator sets take 64 registers, 8 positions spill (44 to 56 bytes of scratch
// in the resource report) and 5 do not - the fanouts 10 and 25 are whole batches of 5.  Byte loads: 2,
// each code has a register of its own until it is packed.
template <int NT, bool VEC>
constexpr int Fp8DenseBatch() { return !VEC ? 2 : NT == 8 ? 5 : 8; }

// W^T of columns f0 .. f0 + 16 NT and of slots k_base .. k_base + k_len into wt; slot k holds row
// Fp8DenseRow(k) of w [k_all, f_all] (permuted) or row k; +0 beyond f_all and k_all
template <int DT, int NT>
__device__ __forceinline__ void Fp8StageW(const void* w, int32_t k_all, int32_t f_all, int32_t f0, int32_t k_base,
                                          int32_t k_len, int32_t stride, bool permuted, unsigned char* wt) {
  constexpr int kCols = 16 * NT;
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  const int32_t total = kCols * k_len;
  for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
    const int32_t c = i % kCols, k = i / kCols;
    const int32_t row = permuted ? Fp8DenseRow(k_base + k) : k_base + k;
    const bool live = row < k_all && f0 + c < f_all;
    const int64_t at = (int64_t)row * f_all + f0 + c;
    unsigned char* to = wt + DenseWtByte(c, k * kEsz, stride);
    if constexpr (DT == kF32)
      *reinterpret_cast<uint32_t*>(to) = live ? static_cast<const uint32_t*>(w)[at] : 0u;
    else
      *reinterpret_cast<uint16_t*>(to) = live ? static_cast<const uint16_t*>(w)[at] : (uint16_t)0;
  }
}

// The sixteen codes k .. k + 16 of the row at byte offset `at` (< 0: no row), zero codes from d on
template <bool VEC>
__device__ __forceinline__ uint4 Fp8DenseLoad(const uint8_t* q, int64_t at, int32_t k, int32_t d) {
  if constexpr (VEC) {          // d % 16 == 0: k < d is k + 16 <= d
    return (at >= 0 && k < d) ? *reinterpret_cast<const uint4*>(q + at + k) : uint4{0u, 0u, 0u, 0u};
  } else {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (at >= 0 && k + j < d) w[j / 4] |= (uint32_t)q[at + k + j] << (8 * (j % 4));
    return uint4{w[0], w[1], w[2], w[3]};
  }
}

// the lane's column scales of a fold tile: columns k + 64 b + i of block b; +0 from d on
__device__ __forceinline__ void Fp8DenseScales(const float* scale, int32_t k, int32_t d, float (*s)[16]) {
#pragma unroll
  for (int b = 0; b < kFp8DenseBlocks; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int32_t col = k + kFp8DenseBlock * b + i;
      s[b][i] = col < d ? scale[col] : 0.f;
    }
}

// fold[0 .. 16) += x^ of the sixteen codes of v, each add rounded on its own; scaled: times rs first
__device__ __forceinline__ void Fp8DenseFoldAdd(const uint4& v, const float* s, float* fold, bool scaled, float rs) {
  float x[16];
  Fp8Value16(v, s, x);
#pragma unroll
  for (int j = 0; j < 16; ++j) fold[j] = MpwAdd(fold[j], scaled ? MpwMul(rs, x[j]) : x[j]);
}

template <int DT>
__device__ __forceinline__ void Fp8DenseStore(const Fp8DenseArgs& a, int64_t at, float v) {
  if (DT == kF32 || a.out_f32) static_cast<float*>(a.out)[at] = v;
  else if constexpr (DT != kF32) static_cast<uint16_t*>(a.out)[at] = HalfCvt<DT>::Narrow(v);
}

extern __shared__ __align__(16) unsigned char fp8_dense_lds[];

template <int DT, int NT, bool VEC>
__global__ __launch_bounds__(64 * kDenseWaves, 2) void Fp8DenseKernel(const Fp8DenseArgs a) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int PB = Fp8DenseBatch<NT, VEC>();
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const bool indexed = a.root_index != nullptr;
  const bool self = a.root_weight != nullptr, fold_root = a.combine == kDenseFold;
  unsigned char* wt_n = fp8_dense_lds;
  unsigned char* wt_s = fp8_dense_lds + 16 * NT * a.plan.stride_n;
  const int32_t d64 = (a.d + kFp8DenseBlock - 1) / kFp8DenseBlock * kFp8DenseBlock;
  // the staged K extent of the self path: an indexed root shares the neighbour path's layout
  const int32_t s_k = !self ? 0 : indexed ? d64 : (a.ds + kPoolChunk - 1) / kPoolChunk * kPoolChunk;
  const bool lock = a.plan.w_tiles > 1;
  const int32_t w_tile = a.plan.w_tile;
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kDenseWaves - 1) / kDenseWaves;
  const bool mean = a.op == kPoolMean;
  const int32_t out_cols = a.combine == kDenseConcat ? a.fs + a.f : a.f;
  const int32_t out_n0 = a.combine == kDenseConcat ? a.fs : 0;
  // one fold tile: its scales are loaded once; beyond, per fold tile
  const bool one_tile = d64 <= kDenseFoldTile;
  float sc[kFp8DenseBlocks][16];
  if (one_tile) Fp8DenseScales(a.scale, 16 * g, a.d, sc);

  for (int32_t fp = 0; fp < a.plan.f_passes; ++fp) {
    const int32_t f0 = fp * 16 * NT;
    if (!lock) {
      __syncthreads();
      if (f0 < a.f) Fp8StageW<DT, NT>(a.weight, a.d, a.f, f0, 0, d64, a.plan.stride_n, true, wt_n);
      if (self && f0 < a.fs) Fp8StageW<DT, NT>(a.root_weight, a.ds, a.fs, f0, 0, s_k, a.plan.stride_s, indexed, wt_s);
      __syncthreads();
    }
    // the bias of column f0 + 16 n + c, the column this lane holds of fragment n
    float bv[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int32_t col = f0 + 16 * n + c;
      bv[n] = 0.f;
      if (a.bias && col < a.f)
        bv[n] = a.bias_f32 ? static_cast<const float*>(a.bias)[col]
                           : TkWiden<DT>(DT == kF32 ? static_cast<const uint32_t*>(a.bias)[col]
                                                    : (uint32_t)static_cast<const uint16_t*>(a.bias)[col]);
    }
    const bool do_n = f0 < a.f, do_s = self && indexed && f0 < a.fs;

    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
      const int64_t r0 = (grp * kDenseWaves + wave) * kPoolTile;
      const int32_t nr = r0 >= a.size ? 0 : (a.size - r0 < kPoolTile ? (int32_t)(a.size - r0) : kPoolTile);
      // this lane's destination: its positions [seg_b, seg_b + len) and its root row
      int64_t seg_b = 0, seg_e = 0;
      if (c < nr) TkSegment(a.seg_ptr, a.count, a.e, r0 + c, &seg_b, &seg_e);
      const int32_t len = (int32_t)(seg_e - seg_b);
      int32_t trips;                              // the run's longest segment, a scalar
      if (a.seg_ptr) {
        int32_t m = len;
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) {
          const int32_t o = __shfl_xor(m, s);
          m = o > m ? o : m;
        }
        trips = __builtin_amdgcn_readfirstlane(m);
      } else {
        trips = nr > 0 ? (int32_t)a.count : 0;
      }
      // dense: the element offset of root[r]; indexed: the byte offset of the row of q it names
      int64_t root_at = -1;
      if (c < nr) {
        if (indexed) {
          const int64_t row = TkRow(a.root_index, a.root_is_ids, r0 + c, a.rows);
          root_at = row < 0 ? -1 : row * a.d;
        } else if (a.root) {
          root_at = (r0 + c) * a.ds;
        }
      }
      const float denom = DenseDenominator((int64_t)len + (fold_root ? 1 : 0));

      DenseAcc acc_n[NT], acc_s[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) acc_n[n] = acc_s[n] = DenseAcc{0.f, 0.f, 0.f, 0.f};

      for (int32_t wk = 0; wk < a.plan.w_tiles; ++wk) {
        const int32_t k_base = wk * w_tile;
        if (lock) {
          __syncthreads();
          if (k_base < d64 && f0 < a.f)
            Fp8StageW<DT, NT>(a.weight, a.d, a.f, f0, k_base, d64 - k_base < w_tile ? d64 - k_base : w_tile,
                              a.plan.stride_n, true, wt_n);
          if (k_base < s_k && f0 < a.fs)
            Fp8StageW<DT, NT>(a.root_weight, a.ds, a.fs, f0, k_base, s_k - k_base < w_tile ? s_k - k_base : w_tile,
                              a.plan.stride_s, indexed, wt_s);
          __syncthreads();
        }
        if (nr == 0) continue;

        // the neighbour path, and with it an indexed root: fold tile by fold tile
        const int32_t n_end = d64 < k_base + w_tile ? d64 : k_base + w_tile;
        if (do_n || do_s) {
#pragma unroll 1
          for (int32_t k0 = k_base; k0 < n_end; k0 += kDenseFoldTile) {
            const int32_t live = (n_end - k0) / kPoolChunk < kDenseChunks ? (n_end - k0) / kPoolChunk : kDenseChunks;
            if (!one_tile) Fp8DenseScales(a.scale, k0 + 16 * g, a.d, sc);
            float fold[kFp8DenseBlocks][16];
#pragma unroll
            for (int b = 0; b < kFp8DenseBlocks; ++b)
#pragma unroll
              for (int j = 0; j < 16; ++j) fold[b][j] = 0.f;
            if (indexed && (fold_root || do_s)) {
              uint4 rv[kFp8DenseBlocks];
#pragma unroll
              for (int b = 0; b < kFp8DenseBlocks; ++b)
                rv[b] = Fp8DenseLoad<VEC>(a.q, root_at, k0 + kFp8DenseBlock * b + 16 * g, a.d);
              if (fold_root) {
#pragma unroll
                for (int b = 0; b < kFp8DenseBlocks; ++b) Fp8DenseFoldAdd(rv[b], sc[b], fold[b], a.has_scale != 0, a.root_scale);
              } else {
#pragma unroll
                for (int b = 0; b < kFp8DenseBlocks; ++b) {
                  float x[16];
                  Fp8Value16(rv[b], sc[b], x);
#pragma unroll
                  for (int j = 0; j < 2; ++j) {
                    if (2 * b + j < live) {
                      DenseWords af[FW];
                      DenseFragment<DT>(x + 8 * j, false, 1.f, af);
                      DenseChunkMma<DT, NT>(af, wt_s, a.plan.stride_s,
                                            (k0 - k_base + (2 * b + j) * kPoolChunk + 8 * g) * kEsz, c, acc_s);
                    }
                  }
                }
              }
            } else if (fold_root) {             // a dense root, read in the blocks' layout
#pragma unroll
              for (int b = 0; b < kFp8DenseBlocks; ++b)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                  DenseWords rw[FW];
                  DenseLoadA<DT, VEC>(a.root, root_at, k0 + kFp8DenseBlock * b + 16 * g + 8 * j, a.d, rw);
                  DenseFoldAdd<DT>(rw, fold[b] + 8 * j, a.has_scale != 0, a.root_scale);
                }
            }
            if (!do_n) continue;
#pragma unroll 1
            for (int32_t j0 = 0; j0 < trips; j0 += PB) {
              int64_t at[PB];
#pragma unroll
              for (int y = 0; y < PB; ++y) {
                const int64_t row = j0 + y < len ? TkRow(a.gather, a.is_ids, seg_b + j0 + y, a.rows) : -1;
                at[y] = row < 0 ? -1 : row * a.d;
              }
              uint4 rv[PB][kFp8DenseBlocks];
#pragma unroll
              for (int y = 0; y < PB; ++y)
#pragma unroll
                for (int b = 0; b < kFp8DenseBlocks; ++b)
                  rv[y][b] = Fp8DenseLoad<VEC>(a.q, at[y], k0 + kFp8DenseBlock * b + 16 * g, a.d);
#pragma unroll
              for (int y = 0; y < PB; ++y)
#pragma unroll
                for (int b = 0; b < kFp8DenseBlocks; ++b) Fp8DenseFoldAdd(rv[y][b], sc[b], fold[b], false, 0.f);
            }
#pragma unroll
            for (int b = 0; b < kFp8DenseBlocks; ++b)
#pragma unroll
              for (int j = 0; j < 2; ++j) {
                if (2 * b + j < live) {
                  DenseWords af[FW];
                  DenseFragment<DT>(fold[b] + 8 * j, mean, denom, af);
                  DenseChunkMma<DT, NT>(af, wt_n, a.plan.stride_n,
                                        (k0 - k_base + (2 * b + j) * kPoolChunk + 8 * g) * kEsz, c, acc_n);
                }
              }
          }
        }

        // a dense root's self path: A fragments straight from the root rows, the plain K order
        const int32_t s_end = s_k < k_base + w_tile ? s_k : k_base + w_tile;
        if (self && !indexed && f0 < a.fs) {
#pragma unroll 1
          for (int32_t k0 = k_base; k0 < s_end; k0 += kDenseFoldTile) {
            const int32_t live = (s_end - k0) / kPoolChunk < kDenseChunks ? (s_end - k0) / kPoolChunk : kDenseChunks;
            DenseWords rw[kDenseChunks][FW];
#pragma unroll
            for (int x = 0; x < kDenseChunks; ++x)
              DenseLoadA<DT, VEC>(a.root, root_at, k0 + x * kPoolChunk + 8 * g, a.ds, rw[x]);
#pragma unroll
            for (int x = 0; x < kDenseChunks; ++x)
              if (x < live)
                DenseChunkMma<DT, NT>(rw[x], wt_s, a.plan.stride_s, (k0 - k_base + x * kPoolChunk + 8 * g) * kEsz, c, acc_s);
          }
        }
      }

      // the epilogue, in the accumulator layout: rows 4 g + i of column c of every fragment
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int32_t col = f0 + 16 * n + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int32_t ri = 4 * g + i;
          if (ri >= nr) continue;
          const int64_t at = (r0 + ri) * out_cols;
          const float vn = PoolAct(a.act, MpwAdd(acc_n[n][i], bv[n]));
          if (a.combine == kDenseConcat) {
            if (col < a.fs) Fp8DenseStore<DT>(a, at + col, PoolAct(a.act, acc_s[n][i]));
            if (col < a.f) Fp8DenseStore<DT>(a, at + out_n0 + col, vn);
          } else if (col < a.f) {
            Fp8DenseStore<DT>(a, at + col, self ? MpwAdd(vn, PoolAct(a.act, acc_s[n][i])) : vn);
          }
        }
      }
    }
  }
}

template <int DT, int NT, bool VEC>
int Fp8DenseLaunch(hipStream_t st, const Fp8DenseArgs& a) {
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kDenseWaves - 1) / kDenseWaves;
  const unsigned blocks = (unsigned)(groups > kDenseMaxBlocks ? kDenseMaxBlocks : groups);
  hipLaunchKernelGGL((Fp8DenseKernel<DT, NT, VEC>), dim3(blocks), dim3(64 * kDenseWaves), (size_t)a.plan.lds_bytes, st,
                     a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT, int NT>
int Fp8DenseDispatchLoads(hipStream_t st, const Fp8DenseArgs& a) {
  const bool vec = Fp8DenseVectorLoads(a.d, (uintptr_t)a.q) &&
                   (!a.root || PoolVectorLoads(a.ds, (uintptr_t)a.root, DT == kF32));
  return vec ? Fp8DenseLaunch<DT, NT, true>(st, a) : Fp8DenseLaunch<DT, NT, false>(st, a);
}

template <int DT>
int Fp8DenseDispatchTile(hipStream_t st, const Fp8DenseArgs& a) {
  switch (a.plan.nt) {
    case 1: return Fp8DenseDispatchLoads<DT, 1>(st, a);
    case 2: return Fp8DenseDispatchLoads<DT, 2>(st, a);
    case 4: return Fp8DenseDispatchLoads<DT, 4>(st, a);
    default: return Fp8DenseDispatchLoads<DT, 8>(st, a);
  }
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_fp8_aggregate_dense(void* stream, int32_t op, int32_t act, int32_t combine, const uint8_t* q_dev,
                                  const float* scale_dev, int64_t rows, int32_t weight_dtype, const void* weight_dev,
                                  const void* bias_dev, int32_t bias_dtype, const void* gather_dev,
                                  int32_t gather_is_ids, const int64_t* seg_ptr_dev, int64_t count, int64_t e,
                                  int64_t d, int64_t f, int64_t size, const void* root_dev, const void* root_index_dev,
                                  int32_t root_index_is_ids, const void* root_weight_dev, int64_t ds, int64_t fs,
                                  int32_t has_root_scale, float root_scale, void* out_dev, int32_t out_dtype) {
  const std::string what("fp8_aggregate_dense");
  if (op != kPoolMean && op != kPoolAdd) return Fail(EULER_GPU_EINVAL, what + ": op is 1 mean, 2 add");
  if (act != kPoolRelu && act != kPoolNone) return Fail(EULER_GPU_EINVAL, what + ": activation is 0 relu, 1 none");
  if (combine < kDenseNone || combine > kDenseFold)
    return Fail(EULER_GPU_EINVAL, what + ": combine is 0 none, 1 add, 2 concat, 3 fold");
  if (!KnownDtype(weight_dtype) || !KnownDtype(out_dtype) || (bias_dev && !KnownDtype(bias_dtype)))
    return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != weight_dtype)
    return Fail(EULER_GPU_EINVAL, what + ": out is fp32 or of the weight's dtype");
  if (bias_dev && bias_dtype != EULER_GPU_F32 && bias_dtype != weight_dtype)
    return Fail(EULER_GPU_EINVAL, what + ": bias is fp32 or of the weight's dtype");
  if (size < 0 || e < 0 || count < 0) return Fail(EULER_GPU_EINVAL, what + ": size, e or count < 0");
  if (e >= (1LL << 31) || size >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, what + ": e or size >= 2^31");
  if (d < 1 || d > kDenseMaxK || f < 1 || f > kDenseMaxF)
    return Fail(EULER_GPU_EINVAL, what + ": d outside 1..1024 or F outside 1..4096");
  const bool two = combine == kDenseAdd || combine == kDenseConcat;
  if (two && (ds < 1 || ds > kDenseMaxK || fs < 1 || fs > kDenseMaxF))
    return Fail(EULER_GPU_EINVAL, what + ": ds outside 1..1024 or Fs outside 1..4096");
  if (combine == kDenseAdd && fs != f) return Fail(EULER_GPU_EINVAL, what + ": combine add needs Fs == F");
  if (combine == kDenseFold && ds != d) return Fail(EULER_GPU_EINVAL, what + ": combine fold needs ds == d");
  if ((seg_ptr_dev != nullptr) == (count > 0))
    return Fail(EULER_GPU_EINVAL, what + ": exactly one of seg_ptr and count");
  if (!seg_ptr_dev && (count >= (1LL << 31) || e != size * count))
    return Fail(EULER_GPU_EINVAL, what + ": count needs e == size * count");
  if (size == 0) return EULER_GPU_OK;
  if (!q_dev || !scale_dev || !weight_dev || !out_dev) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if (root_dev && root_index_dev) return Fail(EULER_GPU_EINVAL, what + ": root or root_index, not both");
  if ((combine != kDenseNone) != (root_dev != nullptr || root_index_dev != nullptr) || two != (root_weight_dev != nullptr))
    return Fail(EULER_GPU_EINVAL, what + ": a root goes with add, concat and fold, root_weight with add and concat");
  if (root_index_dev && ds != d) return Fail(EULER_GPU_EINVAL, what + ": root_index needs ds == d");
  if (rows < 1) return Fail(EULER_GPU_EINVAL, what + ": a table with fewer than 1 row");
  const uintptr_t esz = weight_dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)scale_dev % 4 != 0 || (uintptr_t)weight_dev % esz != 0 || (uintptr_t)root_dev % esz != 0 ||
      (uintptr_t)root_index_dev % (root_index_is_ids ? 8 : 4) != 0 || (uintptr_t)root_weight_dev % esz != 0 ||
      (uintptr_t)bias_dev % (bias_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 4 : 2) != 0 || (uintptr_t)seg_ptr_dev % 8 != 0 ||
      (uintptr_t)gather_dev % (gather_is_ids ? 8 : 4) != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  Fp8DenseArgs a{};
  a.q = q_dev; a.scale = scale_dev; a.rows = rows; a.weight = weight_dev;
  a.bias = bias_dev; a.bias_f32 = bias_dtype == EULER_GPU_F32;
  a.gather = gather_dev; a.is_ids = gather_is_ids != 0;
  a.seg_ptr = seg_ptr_dev; a.count = count; a.e = e;
  a.root = root_dev; a.root_index = root_index_dev; a.root_is_ids = root_index_is_ids != 0;
  a.root_weight = root_weight_dev;
  a.root_scale = root_scale; a.has_scale = combine == kDenseFold && has_root_scale != 0;
  a.d = (int32_t)d; a.f = (int32_t)f; a.size = (int32_t)size; a.op = op; a.act = act; a.combine = combine;
  a.ds = combine == kDenseNone ? 0 : (int32_t)ds;
  a.fs = two ? (int32_t)fs : 0;
  a.out = out_dev; a.out_f32 = out_dtype == EULER_GPU_F32;
  a.plan = Fp8DenseMakePlan(d, two ? ds : 0, root_index_dev != nullptr, two && fs > f ? fs : f,
                            weight_dtype == EULER_GPU_F32);
  hipStream_t st = (hipStream_t)stream;
  if (weight_dtype == EULER_GPU_F32) return Fp8DenseDispatchTile<kF32>(st, a);
  if (weight_dtype == EULER_GPU_BF16) return Fp8DenseDispatchTile<kBF16>(st, a);
  return Fp8DenseDispatchTile<kF16>(st, a);
}

}  // extern "C"
