// Fused gated-graph step (GatedConv: tf_euler/python/convolution/gated_graph_conv.py:26-57) - the
// neighbour sum, then one TF GRUCell - on the matrix units of gfx950, with its C-ABI entry point.
// The contract, the transposed products, the permutation that keeps r * h in registers and the
// phases are stated in mp_gru.h; this file is the kernel and its dispatch ladder.
//
// THE KERNEL, per group of 8 runs (one per wave), the waves in lockstep:
//   fold     lane l folds the segment of destination l % 16 exactly as DenseKernel does and keeps
//            the narrowed sums as the B fragments mf[] of every chunk of the input rows;
//   r pass   the workgroup stages 32 NT columns of the r half of gate_weight over the whole K; the
//            wave multiplies W^T by mf[] and by the h fragments read from its state rows; the
//            epilogue turns each pair of accumulator tiles into one r * h fragment rf[];
//   c pass   16 NT columns of the u half of gate_weight and of cand_weight (state rows permuted)
//            are staged side by side; u from mf[] and h, c from mf[] and rf[]; the blend; the store.
// The fragment arrays are indexed by unrolled loops only: no scratch.  No atomics, no host wait:
// one launch on the caller's stream.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_dense_frag.h"
#include "mp_gru.h"

namespace euler_gpu {
namespace {

// accumulator tiles per gate of a c pass: GruMakePlan's nt
template <int DT, int CH>
constexpr int GruTiles() { return (DT == kF32 ? 8 : 16) / CH; }

struct GruArgs {
  const void* table; int64_t rows;
  const void* state;
  const void* gate_w; const void* cand_w;
  const void* gate_b; int32_t gate_b_f32;
  const void* cand_b; int32_t cand_b_f32;
  const void* gather; int32_t is_ids;
  const int64_t* seg_ptr; int64_t count, e;
  int32_t d, u, size, op;
  void* out; int32_t out_f32;
  GruPlan plan;
};

// Columns col0 .. col0 + COLS of w [d + U, ld] (from col_end on: +0) as Wt[column][slot] over the
// whole staged K: slots 0 .. 32 kd are the input rows, +0 from d on; slots from 32 kd on the state
// rows, +0 from U on - in plain order, or under GruStateRow (permute)
template <int DT, int COLS>
__device__ __forceinline__ void GruStageW(const void* w, int32_t ld, int32_t col0, int32_t col_end, const GruArgs& a,
                                          int32_t stride, bool permute, unsigned char* wt) {
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  const int32_t d32 = kPoolChunk * a.plan.kd, total = COLS * kPoolChunk * (a.plan.kd + a.plan.ku);
  for (int32_t i = threadIdx.x; i < total; i += 64 * kGruWaves) {
    const int32_t c = i % COLS, s = i / COLS;
    int32_t row;                    // of w; -1: +0
    if (s < d32) {
      row = s < a.d ? s : -1;
    } else {
      const int32_t h = permute ? GruStateRow(s - d32) : s - d32;
      row = h < a.u ? a.d + h : -1;
    }
    const bool live = row >= 0 && col0 + c < col_end;
    const int64_t at = (int64_t)row * ld + col0 + c;
    unsigned char* to = wt + DenseWtByte(c, s * kEsz, stride);
    if constexpr (DT == kF32)
      *reinterpret_cast<uint32_t*>(to) = live ? static_cast<const uint32_t*>(w)[at] : 0u;
    else
      *reinterpret_cast<uint16_t*>(to) = live ? static_cast<const uint16_t*>(w)[at] : (uint16_t)0;
  }
}

// acc += Wt (gate columns 16 tile .. + 16 of the staged region, the chunk at slot `slot` + 8 g) x b
template <int DT>
__device__ __forceinline__ DenseAcc GruTileMma(const unsigned char* wt, int32_t stride, int32_t tile, int32_t slot,
                                               int32_t c, const DenseWords* b, DenseAcc acc) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  DenseWords aw[FW];
#pragma unroll
  for (int q = 0; q < FW; ++q)
    aw[q] = *reinterpret_cast<const DenseWords*>(wt + DenseWtByte(tile * 16 + c, slot * kEsz + 16 * q, stride));
  return DenseMma<DT>(aw, b, acc);
}

// element i of a vector of DT (bias: fp32 when f32), widened; +0 when not live (element 0 is read)
template <int DT>
__device__ __forceinline__ float GruElem(const void* p, bool f32, int64_t i, bool live) {
  if (!p) return 0.f;
  const int64_t at = live ? i : 0;
  const float v = (DT == kF32 || f32) ? static_cast<const float*>(p)[at]
                                      : TkWiden<DT>((uint32_t)static_cast<const uint16_t*>(p)[at]);
  return live ? v : 0.f;
}

template <int DT>
__device__ __forceinline__ void GruStore(const GruArgs& a, int64_t at, float v) {
  if (DT == kF32 || a.out_f32) static_cast<float*>(a.out)[at] = v;
  else if constexpr (DT != kF32) static_cast<uint16_t*>(a.out)[at] = HalfCvt<DT>::Narrow(v);
}

// The chunk steps are unrolled so that the fragment arrays stay in registers; without a fence the
// scheduler hoists every LDS read of a pass above the first MFMA and the kernel spills
__device__ __forceinline__ void GruChunkFence() { __builtin_amdgcn_sched_barrier(0); }

// The column stride as a value the compiler takes as new in every pass: the LDS addresses of a pass
// are then formed where they are used, one add each, and not hoisted out of the group loop as some
// hundred loop-invariant registers
__device__ __forceinline__ int32_t GruPassStride(int32_t stride) {
  asm volatile("" : "+s"(stride));
  return stride;
}

extern __shared__ __align__(16) unsigned char gru_lds[];

template <int DT, int CH, bool VEC>
__global__ __launch_bounds__(64 * kGruWaves) void GruKernel(const GruArgs a) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int PB = DenseBatch<DT, VEC>();
  constexpr int NT = GruTiles<DT, CH>();
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const int32_t kd = a.plan.kd, ku = a.plan.ku;
  const int32_t d32 = kPoolChunk * kd;
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kGruWaves - 1) / kGruWaves;
  const bool mean = a.op == kPoolMean;

  for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int64_t r0 = (grp * kGruWaves + wave) * kPoolTile;
    const int32_t nr = r0 >= a.size ? 0 : (a.size - r0 < kPoolTile ? (int32_t)(a.size - r0) : kPoolTile);
    // this lane's destination: its positions [seg_b, seg_b + len) and its state row
    int64_t seg_b = 0, seg_e = 0;
    if (c < nr) TkSegment(a.seg_ptr, a.count, a.e, r0 + c, &seg_b, &seg_e);
    const int32_t len = (int32_t)(seg_e - seg_b);
    int32_t trips;                                // the run's longest segment, a scalar
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
    const int64_t h_at = c < nr ? (r0 + c) * a.u : -1;
    const float denom = DenseDenominator((int64_t)len);

    // ---- the fold: mf[x] = the B fragment of chunk x of m ----
    DenseWords mf[CH][FW], rf[CH][FW];
#pragma unroll
    for (int x = 0; x < CH; ++x)
#pragma unroll
      for (int q = 0; q < FW; ++q) mf[x][q] = DenseWords{0u, 0u, 0u, 0u};
#pragma unroll
    for (int ft = 0; ft < CH / kDenseChunks; ++ft) {
      const int32_t k0 = ft * kDenseFoldTile;
      if (k0 < d32) {
        float fold[kDenseChunks][8];
#pragma unroll
        for (int x = 0; x < kDenseChunks; ++x)
#pragma unroll
          for (int j = 0; j < 8; ++j) fold[x][j] = 0.f;
#pragma unroll 1
        for (int32_t j0 = 0; j0 < trips; j0 += PB) {
          int64_t at[PB];
#pragma unroll
          for (int y = 0; y < PB; ++y) {
            const int64_t row = j0 + y < len ? TkRow(a.gather, a.is_ids, seg_b + j0 + y, a.rows) : -1;
            at[y] = row < 0 ? -1 : row * a.d;
          }
          DenseWords rw[PB][kDenseChunks][FW];
#pragma unroll
          for (int y = 0; y < PB; ++y)
#pragma unroll
            for (int x = 0; x < kDenseChunks; ++x)
              DenseLoadA<DT, VEC>(a.table, at[y], k0 + x * kPoolChunk + 8 * g, a.d, rw[y][x]);
#pragma unroll
          for (int y = 0; y < PB; ++y)
#pragma unroll
            for (int x = 0; x < kDenseChunks; ++x) DenseFoldAdd<DT>(rw[y][x], fold[x], false, 0.f);
        }
#pragma unroll
        for (int x = 0; x < kDenseChunks; ++x) DenseFragment<DT>(fold[x], mean, denom, mf[ft * kDenseChunks + x]);
      }
    }

    // ---- r passes: rf[x] = the B fragment of chunk x of r * h ----
#pragma unroll
    for (int x = 0; x < CH; ++x)
#pragma unroll
      for (int q = 0; q < FW; ++q) rf[x][q] = DenseWords{0u, 0u, 0u, 0u};
#pragma unroll 1
    for (int32_t rp = 0; rp < a.plan.r_passes; ++rp) {
      const int32_t t0 = rp * 2 * NT;                        // first column tile of the pass
      const int32_t stride = GruPassStride(a.plan.stride);
      __syncthreads();
      GruStageW<DT, 32 * NT>(a.gate_w, 2 * a.u, t0 * 16, a.u, a, stride, false, gru_lds);
      __syncthreads();
      if (nr == 0) continue;
      DenseAcc acc[2 * NT];
#pragma unroll
      for (int n = 0; n < 2 * NT; ++n) acc[n] = DenseAcc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int x = 0; x < CH; ++x) {
        if (x < kd) {
#pragma unroll
          for (int n = 0; n < 2 * NT; ++n)
            acc[n] = GruTileMma<DT>(gru_lds, stride, n, x * kPoolChunk + 8 * g, c, mf[x], acc[n]);
        }
        GruChunkFence();
      }
#pragma unroll
      for (int x = 0; x < CH; ++x) {
        if (x < ku) {
          DenseWords hf[FW];
          DenseLoadA<DT, VEC>(a.state, h_at, x * kPoolChunk + 8 * g, a.u, hf);
#pragma unroll
          for (int n = 0; n < 2 * NT; ++n)
            acc[n] = GruTileMma<DT>(gru_lds, stride, n, d32 + x * kPoolChunk + 8 * g, c, hf, acc[n]);
        }
        GruChunkFence();
      }
      // tiles 2 q, 2 q + 1 of the pass: the 8 slots this lane holds of chunk rp NT + q of r * h
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const int32_t xc = rp * NT + q;
        if (xc < ku) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int32_t col = 32 * xc + 16 * (j >> 2) + 4 * g + (j & 3);
            const bool live = col < a.u && c < nr;
            const float r = GruSigmoid(MpwAdd(acc[2 * q + (j >> 2)][j & 3], GruElem<DT>(a.gate_b, a.gate_b_f32 != 0, col, live)));
            v[j] = MpwMul(r, GruElem<DT>(a.state, false, h_at + col, live));
          }
          DenseWords w[FW];
          DenseFragment<DT>(v, false, 1.f, w);
#pragma unroll
          for (int x = 0; x < CH; ++x)
            if (x == xc) {
#pragma unroll
              for (int y = 0; y < FW; ++y) rf[x][y] = w[y];
            }
        }
        GruChunkFence();
      }
    }

    // ---- c passes: u and c of 16 NT columns, the blend, the store ----
#pragma unroll 1
    for (int32_t cp = 0; cp < a.plan.c_passes; ++cp) {
      const int32_t t0 = cp * NT;
      const int32_t stride = GruPassStride(a.plan.stride);
      unsigned char* wt_u = gru_lds;
      unsigned char* wt_c = gru_lds + 16 * NT * stride;
      __syncthreads();
      GruStageW<DT, 16 * NT>(a.gate_w, 2 * a.u, a.u + t0 * 16, 2 * a.u, a, stride, false, wt_u);
      GruStageW<DT, 16 * NT>(a.cand_w, a.u, t0 * 16, a.u, a, stride, true, wt_c);
      __syncthreads();
      if (nr == 0) continue;
      DenseAcc acc_u[NT], acc_c[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) acc_u[n] = acc_c[n] = DenseAcc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int x = 0; x < CH; ++x) {
        if (x < kd) {
#pragma unroll
          for (int n = 0; n < NT; ++n)
            {
              acc_u[n] = GruTileMma<DT>(wt_u, stride, n, x * kPoolChunk + 8 * g, c, mf[x], acc_u[n]);
              acc_c[n] = GruTileMma<DT>(wt_c, stride, n, x * kPoolChunk + 8 * g, c, mf[x], acc_c[n]);
            }
        }
        GruChunkFence();
      }
#pragma unroll
      for (int x = 0; x < CH; ++x) {
        if (x < ku) {
          DenseWords hf[FW];
          DenseLoadA<DT, VEC>(a.state, h_at, x * kPoolChunk + 8 * g, a.u, hf);
#pragma unroll
          for (int n = 0; n < NT; ++n)
            {
              acc_u[n] = GruTileMma<DT>(wt_u, stride, n, d32 + x * kPoolChunk + 8 * g, c, hf, acc_u[n]);
              acc_c[n] = GruTileMma<DT>(wt_c, stride, n, d32 + x * kPoolChunk + 8 * g, c, rf[x], acc_c[n]);
            }
        }
        GruChunkFence();
      }
      // the accumulator layout: columns 16 (t0 + n) + 4 g + i of destination c
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int32_t col = 16 * (t0 + n) + 4 * g + i;
          const bool live = col < a.u && c < nr;
          const float zu = MpwAdd(acc_u[n][i], GruElem<DT>(a.gate_b, a.gate_b_f32 != 0, a.u + col, live));
          const float zc = MpwAdd(acc_c[n][i], GruElem<DT>(a.cand_b, a.cand_b_f32 != 0, col, live));
          const float h = GruElem<DT>(a.state, false, h_at + col, live);
          const float o = GruBlend(GruSigmoid(zu), h, GruTanh(zc));
          if (live) GruStore<DT>(a, h_at + col, o);
        }
        GruChunkFence();
      }
    }
  }
}

template <int DT, int CH, bool VEC>
int GruLaunch(hipStream_t st, const GruArgs& a) {
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kGruWaves - 1) / kGruWaves;
  const unsigned blocks = (unsigned)(groups > kGruMaxBlocks ? kGruMaxBlocks : groups);
  hipLaunchKernelGGL((GruKernel<DT, CH, VEC>), dim3(blocks), dim3(64 * kGruWaves), (size_t)a.plan.lds_bytes, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

// ONE flag selects 16-byte loads for the table's rows and the state's rows alike: a U that is no
// multiple of 8 (fp32: 4), or a state that starts off a 16-byte boundary, sends the gathered rows
// through element loads too, whatever d allows.  Such shapes are served correctly and more slowly
// (DESIGN 4.31); a flag per operand would double the 12 instantiations.
template <int DT>
int GruDispatch(hipStream_t st, const GruArgs& a) {
  const bool vec = PoolVectorLoads(a.d, (uintptr_t)a.table, DT == kF32) &&
                   PoolVectorLoads(a.u, (uintptr_t)a.state, DT == kF32);
  if (a.plan.ch == 4) return vec ? GruLaunch<DT, 4, true>(st, a) : GruLaunch<DT, 4, false>(st, a);
  return vec ? GruLaunch<DT, 8, true>(st, a) : GruLaunch<DT, 8, false>(st, a);
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_aggregate_gru(void* stream, int32_t op, const void* table_dev, int32_t dtype, int64_t rows,
                            const void* gather_dev, int32_t gather_is_ids, const int64_t* seg_ptr_dev, int64_t count,
                            int64_t e, int64_t d, int64_t u, int64_t size, const void* state_dev,
                            const void* gate_weight_dev, const void* cand_weight_dev, const void* gate_bias_dev,
                            int32_t gate_bias_dtype, const void* cand_bias_dev, int32_t cand_bias_dtype, void* out_dev,
                            int32_t out_dtype) {
  const std::string what("aggregate_gru");
  if (op != kPoolMean && op != kPoolAdd) return Fail(EULER_GPU_EINVAL, what + ": op is 1 mean, 2 add");
  if (!KnownDtype(dtype) || !KnownDtype(out_dtype) || (gate_bias_dev && !KnownDtype(gate_bias_dtype)) ||
      (cand_bias_dev && !KnownDtype(cand_bias_dtype)))
    return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != dtype)
    return Fail(EULER_GPU_EINVAL, what + ": out is fp32 or of the table's dtype");
  if ((gate_bias_dev && gate_bias_dtype != EULER_GPU_F32 && gate_bias_dtype != dtype) ||
      (cand_bias_dev && cand_bias_dtype != EULER_GPU_F32 && cand_bias_dtype != dtype))
    return Fail(EULER_GPU_EINVAL, what + ": a bias is fp32 or of the table's dtype");
  if (size < 0 || e < 0 || count < 0) return Fail(EULER_GPU_EINVAL, what + ": size, e or count < 0");
  if (e >= (1LL << 31) || size >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, what + ": e or size >= 2^31");
  if (d < 1 || d > kGruMaxD || u < 1 || u > kGruMaxU)
    return Fail(EULER_GPU_EINVAL, what + ": d outside 1..256 or U outside 1..256");
  if ((seg_ptr_dev != nullptr) == (count > 0))
    return Fail(EULER_GPU_EINVAL, what + ": exactly one of seg_ptr and count");
  if (!seg_ptr_dev && (count >= (1LL << 31) || e != size * count))
    return Fail(EULER_GPU_EINVAL, what + ": count needs e == size * count");
  if (size == 0) return EULER_GPU_OK;
  if (!table_dev || !state_dev || !gate_weight_dev || !cand_weight_dev || !out_dev)
    return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if (rows < 1) return Fail(EULER_GPU_EINVAL, what + ": a table with fewer than 1 row");
  const uintptr_t esz = dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)table_dev % esz != 0 || (uintptr_t)state_dev % esz != 0 || (uintptr_t)gate_weight_dev % esz != 0 ||
      (uintptr_t)cand_weight_dev % esz != 0 || (uintptr_t)gate_bias_dev % (gate_bias_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)cand_bias_dev % (cand_bias_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 4 : 2) != 0 || (uintptr_t)seg_ptr_dev % 8 != 0 ||
      (uintptr_t)gather_dev % (gather_is_ids ? 8 : 4) != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  GruArgs a{};
  a.table = table_dev; a.rows = rows; a.state = state_dev;
  a.gate_w = gate_weight_dev; a.cand_w = cand_weight_dev;
  a.gate_b = gate_bias_dev; a.gate_b_f32 = gate_bias_dtype == EULER_GPU_F32;
  a.cand_b = cand_bias_dev; a.cand_b_f32 = cand_bias_dtype == EULER_GPU_F32;
  a.gather = gather_dev; a.is_ids = gather_is_ids != 0;
  a.seg_ptr = seg_ptr_dev; a.count = count; a.e = e;
  a.d = (int32_t)d; a.u = (int32_t)u; a.size = (int32_t)size; a.op = op;
  a.out = out_dev; a.out_f32 = out_dtype == EULER_GPU_F32;
  a.plan = GruMakePlan(d, u, dtype == EULER_GPU_F32);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EULER_GPU_F32) return GruDispatch<kF32>(st, a);
  if (dtype == EULER_GPU_BF16) return GruDispatch<kBF16>(st, a);
  return GruDispatch<kF16>(st, a);
}

}  // extern "C"
