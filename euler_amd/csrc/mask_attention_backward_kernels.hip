// The gradient of mask_attention on the matrix units of gfx950, and its C-ABI entry point.  The
// contract, the arithmetic and the order of every sum are stated in mp_mask_attention_backward.h; this
// file is the two kernels and the dispatch ladder.
//
// KERNEL 1, per work item (batch row, source tile, head): the forward's pass 1 for the shift; then per
// column tile of the head the forward's pass 2 with every numerator split by the sign of its
// pre-activation into two A fragments and two accumulator sets (ONE B read for both runs and both
// fragments), and an epilogue in the accumulator layout that carries three dot products with the gated
// gradient per row across the tiles; at the end the 16 column lanes are summed by a fixed exchange
// order and d s_src, d s_root and the statistics of kernel 2 are written.  d root is written per tile.
// KERNEL 2, per work item (batch row, candidate tile, head), over the transposed mask: per source block
// it stages the gated gradient divided by its source's denominator as the B operand and three scalars
// per source, rebuilds the forward's numerators with the roles swapped, and writes d z and d s_nb.
// No atomics, no scratch, no host wait: two launches on the caller's stream.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_mask_attention_backward.h"
#include "mp_mask_attention_frag.h"

namespace euler_gpu {
namespace {

struct MaskAttBwdArgs {
  MaskAttArgs f;            // kernel 1's view, the forward's: f.out is the SAVED output, f.out_f32 the dtype of grad and out
  const void* grad;
  float* stats;             // [batch * n, H, kMaskAttStats]
  float* d_s_src;
  float* d_s_root;
  void* d_root;
  const uint64_t* mask_t;   // kernel 2: [batch * m, words_t]
  void* d_z;
  float* d_s_nb;
  int32_t words_t, waves_t;
  MaskAttPlan plan_t;
};

// the incoming gradient at element `at`, zeroed where the saved output did not pass the relu
template <int DT>
__device__ __forceinline__ float BwdGrad(const MaskAttBwdArgs& a, int64_t at) {
  float g = 0.f, o = 1.f;
  if (DT == kF32 || a.f.out_f32) {
    g = static_cast<const float*>(a.grad)[at];
    if (a.f.relu) o = static_cast<const float*>(a.f.out)[at];
  } else if constexpr (DT != kF32) {
    g = HalfCvt<DT>::Widen(static_cast<const uint16_t*>(a.grad)[at]);
    if (a.f.relu) o = HalfCvt<DT>::Widen(static_cast<const uint16_t*>(static_cast<const void*>(a.f.out))[at]);
  }
  return o <= 0.f ? 0.f : g;
}

// elements k .. k + 8 of the row at element offset `at` (< 0: no row) of an fp32 or DT table, +0 from dh on
template <int DT, bool VEC>
__device__ __forceinline__ void BwdLoad8(const void* table, bool f32, int64_t at, int32_t k, int32_t dh, float* v) {
  if (DT == kF32 || f32) {
    DenseWords r[2];
    DenseLoadA<kF32, VEC>(table, at, k, dh, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = BitsF32(r[j / 4][j % 4]);
  } else if constexpr (DT != kF32) {
    DenseWords r;
    DenseLoadA<DT, VEC>(table, at, k, dh, &r);
#pragma unroll
    for (int j = 0; j < 4; ++j) Widen2<DT>(r[j], &v[2 * j], &v[2 * j + 1]);
  }
}

// The two A fragments of a chunk from its split numerators, each rounded once to the operand type,
// and the rounded values back in fp32 for the scalar sums
template <int DT>
__device__ __forceinline__ void BwdPack(const float* pp, const float* pn, DenseWords* afp, DenseWords* afn, float* rp,
                                        float* rn) {
  if constexpr (DT == kF32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      afp[j / 4][j % 4] = F32Bits(pp[j]);
      afn[j / 4][j % 4] = F32Bits(pn[j]);
      rp[j] = pp[j];
      rn[j] = pn[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      afp[0][j] = Narrow2<DT>(pp[2 * j], pp[2 * j + 1]);
      afn[0][j] = Narrow2<DT>(pn[2 * j], pn[2 * j + 1]);
      Widen2<DT>(afp[0][j], &rp[2 * j], &rp[2 * j + 1]);
      Widen2<DT>(afn[0][j], &rn[2 * j], &rn[2 * j + 1]);
    }
  }
}

// one numerator, split: the forward's p by the forward's arithmetic, selected by its bit, on the side of its sign
__device__ __forceinline__ void BwdNumerator(bool bit, float s_src, float s_nb, float shift, float slope, float* pp,
                                             float* pn) {
  const float pre = MpwAdd(s_src, s_nb);
  const bool neg = pre < 0.f;
  const float pv = bit ? AttExp(neg ? MpwMul(pre, slope) : pre, shift) : 0.f;
  *pp = neg ? 0.f : pv;
  *pn = neg ? pv : 0.f;
}

// the 16 column lanes of a row, by exchanges at lane distance 1, 2, 4, 8: every lane ends with the sum
__device__ __forceinline__ float BwdSumColumns(float v) {
  v = MpwAdd(v, __shfl_xor(v, 1));
  v = MpwAdd(v, __shfl_xor(v, 2));
  v = MpwAdd(v, __shfl_xor(v, 4));
  return MpwAdd(v, __shfl_xor(v, 8));
}

// the four lane groups of source (candidate) c in order: every lane ends with the sum of its column's source
__device__ __forceinline__ float BwdSumGroups(float v, int32_t c) {
  return MpwAdd(MpwAdd(MpwAdd(__shfl(v, c), __shfl(v, c + 16)), __shfl(v, c + 32)), __shfl(v, c + 48));
}

extern __shared__ __align__(16) unsigned char mask_att_bwd_lds[];

// ---- kernel 1: source-major ---------------------------------------------------------------------
template <int DT, int NT, bool VEC>
__global__ __launch_bounds__(64 * kMaskWaves, 2) void MaskAttBwdSourceKernel(const MaskAttBwdArgs args) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int KW = AttBlockWords<DT>();
  const MaskAttArgs& a = args.f;
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const int32_t tile = a.waves * kMaskRuns * kPoolTile;
  const int64_t tiles = ((int64_t)a.n + tile - 1) / tile;
  const int64_t items = a.batch * tiles * a.heads;
  const int32_t stride = a.plan.stride;
  const uint64_t tail = a.m % 64 ? (1ull << (a.m % 64)) - 1ull : ~0ull;   // the live bits of the last word
  float* sc = reinterpret_cast<float*>(mask_att_bwd_lds + a.plan.score_off);

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int32_t h = (int32_t)(item % a.heads);
    const int64_t b = item / a.heads / tiles;
    const int32_t s0 = (int32_t)(item / a.heads % tiles) * tile + wave * kMaskRuns * kPoolTile;
    const int32_t col0 = h * a.dh;
    // this lane's source of each run: its mask row and its scores, or none
    const uint64_t* mrow[kMaskRuns];
    float s_src[kMaskRuns], e0[kMaskRuns], lam0[kMaskRuns], mx[kMaskRuns];
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q) {
      const int32_t src = s0 + q * kPoolTile + c;
      const bool on = src < a.n;
      mrow[q] = on ? a.mask + (b * a.n + src) * (int64_t)a.words : nullptr;
      s_src[q] = on ? a.s_src[(b * a.n + src) * a.heads + h] : 0.f;
      const float s_self = (a.s_root && on) ? a.s_root[(b * a.n + src) * a.heads + h] : 0.f;
      e0[q] = a.s_root ? AttAdditiveLogit(s_src[q], s_self, a.slope) : 0.f;
      lam0[q] = MpwAdd(s_src[q], s_self) < 0.f ? a.slope : 1.f;
      mx[q] = -__builtin_inff();
    }

    // pass 1, the forward's: the largest neighbour score of every source
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
    float shift[kMaskRuns];
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q) {
      float v = mx[q];
      const float v16 = __shfl_xor(v, 16);
      v = v16 > v ? v16 : v;
      const float v32 = __shfl_xor(v, 32);
      v = v32 > v ? v32 : v;
      // (no neighbour: the shift stays -inf, never leaky(-inf), and every p is selected to +0)
      shift[q] = v > -__builtin_inff() ? AttAdditiveLogit(s_src[q], v, a.slope) : v;
      if (a.s_root) shift[q] = e0[q] > shift[q] ? e0[q] : shift[q];
    }

    float lp[kMaskRuns] = {0.f, 0.f}, ln[kMaskRuns] = {0.f, 0.f};          // this lane's partial l+ and l-
    float tp[kMaskRuns], tn[kMaskRuns], p0[kMaskRuns], lt[kMaskRuns];      // of source c, from the first tile on
    float dA[kMaskRuns][4], dS[kMaskRuns][4], dR[kMaskRuns][4];            // the dot products of rows 4 g + i
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) dA[q][i] = dS[q][i] = dR[q][i] = 0.f;

    for (int32_t ct = 0; ct < a.plan.col_tiles; ++ct) {
      const int32_t f0 = ct * 16 * NT;
      const bool first = ct == 0;
      DenseAcc accp[kMaskRuns][NT], accn[kMaskRuns][NT];
#pragma unroll
      for (int q = 0; q < kMaskRuns; ++q)
#pragma unroll
        for (int nf = 0; nf < NT; ++nf) accp[q][nf] = accn[q][nf] = DenseAcc{0.f, 0.f, 0.f, 0.f};

      // pass 2: the split numerators in registers, their sums beside them, products on the matrix units
      for (int64_t c64 = 0; c64 < a.m; c64 += a.plan.kb) {
        const int32_t c0 = (int32_t)c64, w0 = c0 / 64;
        const int32_t live = a.words - w0 < a.plan.kb / 64 ? a.words - w0 : a.plan.kb / 64;
        uint64_t word[kMaskRuns][KW];
        // (element loads keep 64 values in flight while staging: the words come after it, not across it)
        if constexpr (VEC) AttLoadWords<KW>(mrow, w0, live, a.words, tail, word);
        __syncthreads();                           // the previous block's reads (pass 1's, the last tile's) are done
        AttStage<DT, NT, VEC>(a, b * a.m, col0, c0, f0, mask_att_bwd_lds);
        AttStageScores(a, b * a.m, h, c0, sc);
        if constexpr (!VEC) AttLoadWords<KW>(mrow, w0, live, a.words, tail, word);
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
            DenseWords afp[kMaskRuns][FW], afn[kMaskRuns][FW];
#pragma unroll
            for (int q = 0; q < kMaskRuns; ++q) {
              if (!any[q]) continue;
              const uint32_t half = (uint32_t)(word[q][w] >> (32 * x));
              float pp[8], pn[8], rp[8], rn[8];
#pragma unroll
              for (int j = 0; j < 8; ++j)
                BwdNumerator(AttBit<DT>(half, g, j), s_src[q], s[j], shift[q], a.slope, &pp[j], &pn[j]);
              BwdPack<DT>(pp, pn, afp[q], afn[q], rp, rn);
              if (first) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                  lp[q] = MpwAdd(lp[q], rp[j]);
                  ln[q] = MpwAdd(ln[q], rn[j]);
                }
              }
            }
#pragma unroll
            for (int nf = 0; nf < NT; ++nf) {
              DenseWords bw[FW];
              MaskLoadB<DT>(mask_att_bwd_lds, stride, 64 * w + 32 * x, nf, c, g, bw);
#pragma unroll
              for (int q = 0; q < kMaskRuns; ++q) {
                if (!any[q]) continue;
                accp[q][nf] = DenseMma<DT>(afp[q], bw, accp[q][nf]);
                accn[q][nf] = DenseMma<DT>(afn[q], bw, accn[q][nf]);
              }
            }
          }
        }
      }

      // the tile's epilogue, in the accumulator layout: rows 4 g + i of column c of every fragment
#pragma unroll
      for (int q = 0; q < kMaskRuns; ++q) {
        const int32_t r0 = s0 + q * kPoolTile;
        if (first) {
          tp[q] = BwdSumGroups(lp[q], c);
          tn[q] = BwdSumGroups(ln[q], c);
          p0[q] = a.s_root ? AttExp(e0[q], shift[q]) : 0.f;
          lt[q] = MpwAdd(tp[q], tn[q]);
          if (a.s_root) lt[q] = MpwAdd(lt[q], p0[q]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float den = MaskAttDenominator(__shfl(lt[q], 4 * g + i));      // lane 4 g + i holds source 4 g + i of the run
          const float self = __shfl(p0[q], 4 * g + i);
          const int32_t src = r0 + 4 * g + i;
          if (src >= a.n) continue;
          const int64_t at = (b * a.n + src) * a.d + col0;
#pragma unroll
          for (int nf = 0; nf < NT; ++nf) {
            const int32_t col = f0 + 16 * nf + c;
            if (col >= a.dh) continue;
            const float gv = BwdGrad<DT>(args, at + col);
            const float root = a.root ? MaskRoot<DT>(a.root, at + col) : 0.f;
            const float ap = accp[q][nf][i], an = accn[q][nf][i];
            float sum = MpwAdd(ap, an);
            if (a.s_root) {
              sum = MpwAdd(sum, MpwMul(self, root));
              dR[q][i] = MpwAdd(dR[q][i], MpwMul(gv, root));
            }
            dA[q][i] = MpwAdd(dA[q][i], MpwMul(gv, sum));
            dS[q][i] = MpwAdd(dS[q][i], MpwMul(gv, MpwAdd(ap, MpwMul(a.slope, an))));
            if (args.d_root) {
              const float v = a.s_root ? MpwMul(MpwDiv(self, den), gv) : gv;
              if constexpr (DT == kF32) static_cast<float*>(args.d_root)[at + col] = v;
              else static_cast<uint16_t*>(args.d_root)[at + col] = HalfCvt<DT>::Narrow(v);
            }
          }
        }
      }
    }

    // the 16 column lanes of every row, then the scalars of the row from the lane that holds its source
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q) {
      const int32_t r0 = s0 + q * kPoolTile;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float sA = BwdSumColumns(dA[q][i]), sS = BwdSumColumns(dS[q][i]), sR = BwdSumColumns(dR[q][i]);
        const int32_t from = 4 * g + i;
        const float den = MaskAttDenominator(__shfl(lt[q], from));
        const float self = __shfl(p0[q], from), lam = __shfl(lam0[q], from);
        const float lpos = __shfl(tp[q], from), lneg = __shfl(tn[q], from);
        const float own = __shfl(s_src[q], from), top = __shfl(shift[q], from);
        const int32_t src = r0 + from;
        if (c != 0 || src >= a.n) continue;
        const int64_t at = (b * a.n + src) * a.heads + h;
        const float D = MpwDiv(sA, den);
        const float d_self = a.s_root ? MpwDiv(MpwMul(MpwMul(self, lam), MpwSub(sR, D)), den) : 0.f;
        const float d_own = MpwAdd(MpwDiv(MpwSub(sS, MpwMul(D, MpwAdd(lpos, MpwMul(a.slope, lneg)))), den), d_self);
        if (args.d_s_src) args.d_s_src[at] = d_own;
        if (args.d_s_root) args.d_s_root[at] = d_self;
        float* st = args.stats + at * kMaskAttStats;
        st[0] = own;
        st[1] = top;
        st[2] = den;
        st[3] = MpwDiv(D, den);
      }
    }
  }
}

// ---- kernel 2: candidate-major ------------------------------------------------------------------
// The block's slice of the gated gradient of the head's columns, each row divided by its source's
// denominator and rounded once to the operand type, into LDS in AttStage's layout.  Sources i0 + k < n
// of batch row b (row0 = b * n) and columns f0 + f < dh of the head; +0 else
template <int DT, int NT, bool VEC>
__device__ __forceinline__ void BwdStageGrad(const MaskAttBwdArgs& a, int64_t row0, int32_t h, int32_t col0, int32_t i0,
                                             int32_t f0, unsigned char* lds) {
  constexpr int kPieces = 2 * NT;                  // pieces of 8 columns in the column tile
  const int32_t stride = a.plan_t.stride;
  const bool f32 = a.f.out_f32 != 0;
  auto row8 = [&](int32_t src, int32_t k, float* v) {
    const bool on = src < a.f.n;
    const int64_t at = on ? (row0 + src) * a.f.d + col0 : -1;
    BwdLoad8<DT, VEC>(a.grad, f32, at, k, a.f.dh, v);
    if (a.f.relu) {
      float o[8];
      BwdLoad8<DT, VEC>(a.f.out, f32, at, k, a.f.dh, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = o[j] <= 0.f ? 0.f : v[j];
    }
    const float den = on ? a.stats[((row0 + src) * a.f.heads + h) * kMaskAttStats + 2] : 1.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = MpwDiv(v[j], den);
  };
  if constexpr (DT == kF32) {
    const int32_t total = a.plan_t.kb * kPieces;
    for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
      const int32_t fb = i % kPieces, k = i / kPieces;
      float v[8];
      row8(i0 + k, f0 + 8 * fb, v);
      DenseWords* to = reinterpret_cast<DenseWords*>(lds + k * stride + fb * 32);
      to[0] = DenseWords{F32Bits(v[0]), F32Bits(v[1]), F32Bits(v[2]), F32Bits(v[3])};
      to[1] = DenseWords{F32Bits(v[4]), F32Bits(v[5]), F32Bits(v[6]), F32Bits(v[7])};
    }
  } else {
    const int32_t total = (a.plan_t.kb / 8) * kPieces;
    for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
      const int32_t fb = i % kPieces, kblk = i / kPieces;
      DenseWords r[8];                             // r[k][p]: columns 2 p, 2 p + 1 of source k
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float v[8];
        row8(i0 + 8 * kblk + k, f0 + 8 * fb, v);
#pragma unroll
        for (int p = 0; p < 4; ++p) r[k][p] = Narrow2<DT>(v[2 * p], v[2 * p + 1]);
      }
#pragma unroll
      for (int f = 0; f < 8; ++f) {                // column f of the block: sources 2 q, 2 q + 1 per word
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

// s_src, M and D / den of the block's sources into LDS, in source order; +0 from n on
__device__ __forceinline__ void BwdStageStats(const MaskAttBwdArgs& a, int64_t row0, int32_t h, int32_t i0, float* sc) {
  const int32_t kb = a.plan_t.kb;
  for (int32_t i = threadIdx.x; i < kb; i += blockDim.x) {
    const bool on = i0 + i < a.f.n;
    const float* st = a.stats + ((row0 + i0 + i) * a.f.heads + h) * kMaskAttStats;
    sc[i] = on ? st[0] : 0.f;
    sc[kb + i] = on ? st[1] : 0.f;
    sc[2 * kb + i] = on ? st[3] : 0.f;
  }
}

template <int DT, int NT, bool VEC>
__global__ __launch_bounds__(64 * kMaskWaves, 2) void MaskAttBwdCandidateKernel(const MaskAttBwdArgs a) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int KW = AttBlockWords<DT>();
  const int32_t n = a.f.n, m = a.f.m, heads = a.f.heads, dh = a.f.dh, d = a.f.d, kb = a.plan_t.kb;
  const float slope = a.f.slope;
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const int32_t tile = a.waves_t * kMaskRuns * kPoolTile;
  const int64_t tiles = ((int64_t)m + tile - 1) / tile;
  const int64_t items = a.f.batch * tiles * heads;
  const int32_t stride = a.plan_t.stride;
  const uint64_t tail = n % 64 ? (1ull << (n % 64)) - 1ull : ~0ull;       // the live bits of the last word
  float* sc = reinterpret_cast<float*>(mask_att_bwd_lds + a.plan_t.score_off);

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int32_t h = (int32_t)(item % heads);
    const int64_t b = item / heads / tiles;
    const int32_t s0 = (int32_t)(item / heads % tiles) * tile + wave * kMaskRuns * kPoolTile;
    const int32_t col0 = h * dh;
    // this lane's candidate of each run: its row of the transposed mask and its score, or none
    const uint64_t* mrow[kMaskRuns];
    float s_nb[kMaskRuns], wp[kMaskRuns] = {0.f, 0.f}, wn[kMaskRuns] = {0.f, 0.f}, dot[kMaskRuns][4];
#pragma unroll
    for (int q = 0; q < kMaskRuns; ++q) {
      const int32_t cand = s0 + q * kPoolTile + c;
      const bool on = cand < m;
      mrow[q] = on ? a.mask_t + (b * m + cand) * (int64_t)a.words_t : nullptr;
      s_nb[q] = on ? a.f.s_nb[(b * m + cand) * heads + h] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) dot[q][i] = 0.f;
    }

    for (int32_t ct = 0; ct < a.plan_t.col_tiles; ++ct) {
      const int32_t f0 = ct * 16 * NT;
      const bool first = ct == 0;
      DenseAcc accp[kMaskRuns][NT], accn[kMaskRuns][NT];
#pragma unroll
      for (int q = 0; q < kMaskRuns; ++q)
#pragma unroll
        for (int nf = 0; nf < NT; ++nf) accp[q][nf] = accn[q][nf] = DenseAcc{0.f, 0.f, 0.f, 0.f};

      for (int64_t i64 = 0; i64 < n; i64 += kb) {              // (64 bits: n + kb may pass 2^31)
        const int32_t i0 = (int32_t)i64, w0 = i0 / 64;
        const int32_t live = a.words_t - w0 < kb / 64 ? a.words_t - w0 : kb / 64;
        uint64_t word[kMaskRuns][KW];
        AttLoadWords<KW>(mrow, w0, live, a.words_t, tail, word);
        __syncthreads();                           // the previous block's reads are done
        BwdStageGrad<DT, NT, VEC>(a, b * n, h, col0, i0, f0, mask_att_bwd_lds);
        BwdStageStats(a, b * n, h, i0, sc);
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
            float own[8], top[8], dd[8];           // s_src, M and D / den of the lane's eight sources
            AttScores<DT>(sc, 64 * w + 32 * x, g, own);
            AttScores<DT>(sc + kb, 64 * w + 32 * x, g, top);
            if (first) AttScores<DT>(sc + 2 * kb, 64 * w + 32 * x, g, dd);
            DenseWords afp[kMaskRuns][FW], afn[kMaskRuns][FW];
#pragma unroll
            for (int q = 0; q < kMaskRuns; ++q) {
              if (!any[q]) continue;
              const uint32_t half = (uint32_t)(word[q][w] >> (32 * x));
              float pp[8], pn[8], rp[8], rn[8];
#pragma unroll
              for (int j = 0; j < 8; ++j)
                BwdNumerator(AttBit<DT>(half, g, j), own[j], s_nb[q], top[j], slope, &pp[j], &pn[j]);
              BwdPack<DT>(pp, pn, afp[q], afn[q], rp, rn);
              if (first) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                  wp[q] = MpwAdd(wp[q], MpwMul(rp[j], dd[j]));
                  wn[q] = MpwAdd(wn[q], MpwMul(rn[j], dd[j]));
                }
              }
            }
#pragma unroll
            for (int nf = 0; nf < NT; ++nf) {
              DenseWords bw[FW];
              MaskLoadB<DT>(mask_att_bwd_lds, stride, 64 * w + 32 * x, nf, c, g, bw);
#pragma unroll
              for (int q = 0; q < kMaskRuns; ++q) {
                if (!any[q]) continue;
                accp[q][nf] = DenseMma<DT>(afp[q], bw, accp[q][nf]);
                accn[q][nf] = DenseMma<DT>(afn[q], bw, accn[q][nf]);
              }
            }
          }
        }
      }

      // the tile's epilogue, in the accumulator layout: candidates 4 g + i, column c of every fragment
#pragma unroll
      for (int q = 0; q < kMaskRuns; ++q) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int32_t cand = s0 + q * kPoolTile + 4 * g + i;
          if (cand >= m) continue;
          const int64_t at = (b * m + cand) * d + col0;
#pragma unroll
          for (int nf = 0; nf < NT; ++nf) {
            const int32_t col = f0 + 16 * nf + c;
            if (col >= dh) continue;
            const float ap = accp[q][nf][i], an = accn[q][nf][i];
            if (a.d_z) {
              const float v = MpwAdd(ap, an);
              if constexpr (DT == kF32) static_cast<float*>(a.d_z)[at + col] = v;
              else static_cast<uint16_t*>(a.d_z)[at + col] = HalfCvt<DT>::Narrow(v);
            }
            dot[q][i] = MpwAdd(dot[q][i], MpwMul(MaskRoot<DT>(a.f.z, at + col), MpwAdd(ap, MpwMul(slope, an))));
          }
        }
      }
    }

    if (a.d_s_nb) {                                // (uniform: every lane takes part in the exchanges)
#pragma unroll
      for (int q = 0; q < kMaskRuns; ++q) {
        const float tp = BwdSumGroups(wp[q], c), tn = BwdSumGroups(wn[q], c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float sum = BwdSumColumns(dot[q][i]);
          const float wpos = __shfl(tp, 4 * g + i), wneg = __shfl(tn, 4 * g + i);
          const int32_t cand = s0 + q * kPoolTile + 4 * g + i;
          if (c != 0 || cand >= m) continue;
          a.d_s_nb[(b * m + cand) * heads + h] = MpwSub(sum, MpwAdd(wpos, MpwMul(slope, wneg)));
        }
      }
    }
  }
}

template <int DT, int NT>
int BwdLaunch(hipStream_t st, const MaskAttBwdArgs& a, bool vec_z, bool vec_g, bool candidates) {
  const MaskAttArgs& f = a.f;
  {
    const int64_t tile = MaskTile(f.waves);
    const int64_t items = f.batch * ((f.n + tile - 1) / tile) * f.heads;
    const unsigned blocks = (unsigned)(items > kMaskMaxBlocks ? kMaskMaxBlocks : items);
    if (vec_z)
      hipLaunchKernelGGL((MaskAttBwdSourceKernel<DT, NT, true>), dim3(blocks), dim3(64 * f.waves), (size_t)f.plan.lds_bytes, st, a);
    else
      hipLaunchKernelGGL((MaskAttBwdSourceKernel<DT, NT, false>), dim3(blocks), dim3(64 * f.waves), (size_t)f.plan.lds_bytes, st, a);
    EG_HIP(hipGetLastError());
  }
  if (candidates) {
    const int64_t tile = MaskTile(a.waves_t);
    const int64_t items = f.batch * ((f.m + tile - 1) / tile) * f.heads;
    const unsigned blocks = (unsigned)(items > kMaskMaxBlocks ? kMaskMaxBlocks : items);
    if (vec_g)
      hipLaunchKernelGGL((MaskAttBwdCandidateKernel<DT, NT, true>), dim3(blocks), dim3(64 * a.waves_t), (size_t)a.plan_t.lds_bytes, st, a);
    else
      hipLaunchKernelGGL((MaskAttBwdCandidateKernel<DT, NT, false>), dim3(blocks), dim3(64 * a.waves_t), (size_t)a.plan_t.lds_bytes, st, a);
    EG_HIP(hipGetLastError());
  }
  return EULER_GPU_OK;
}

template <int DT>
int BwdDispatchTile(hipStream_t st, const MaskAttBwdArgs& a, bool vec_z, bool vec_g, bool candidates) {
  return a.f.plan.nt == 1 ? BwdLaunch<DT, 1>(st, a, vec_z, vec_g, candidates) : BwdLaunch<DT, 2>(st, a, vec_z, vec_g, candidates);
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" int euler_gpu_mask_attention_backward(void* stream, const uint64_t* mask_dev, const uint64_t* mask_t_dev,
                                                 const void* z_dev, int32_t dtype, int64_t z_rows, const float* s_src_dev,
                                                 const float* s_nb_dev, int64_t s_nb_rows, const void* root_dev,
                                                 const float* s_root_dev, const void* out_dev, const void* grad_dev,
                                                 int32_t grad_dtype, int64_t batch, int64_t n, int64_t m, int64_t d,
                                                 int64_t heads, float negative_slope, int32_t activation, float* stats_ws_dev,
                                                 void* d_z_dev, float* d_s_src_dev, float* d_s_nb_dev, void* d_root_dev,
                                                 float* d_s_root_dev) {
  constexpr int64_t kBig = 1LL << 31;
  const std::string what("mask_attention_backward");
  if (!KnownDtype(dtype) || !KnownDtype(grad_dtype)) return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (grad_dtype != EULER_GPU_F32 && grad_dtype != dtype) return Fail(EULER_GPU_EINVAL, what + ": grad is fp32 or of z's dtype");
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
  if (d_root_dev && !root_dev) return Fail(EULER_GPU_EINVAL, what + ": d_root goes with root only");
  if (d_s_root_dev && !s_root_dev) return Fail(EULER_GPU_EINVAL, what + ": d_s_root goes with s_root only");
  if (activation == kMaskAttRelu && !out_dev) return Fail(EULER_GPU_EINVAL, what + ": relu needs the saved forward output");
  if (batch * n == 0) return EULER_GPU_OK;
  if (!d_z_dev && !d_s_src_dev && !d_s_nb_dev && !d_root_dev && !d_s_root_dev) return EULER_GPU_OK;
  const bool candidates = m > 0 && (d_z_dev || d_s_nb_dev);
  if ((m > 0 && (!mask_dev || !z_dev || !s_nb_dev)) || (candidates && !mask_t_dev) || !s_src_dev || !grad_dev || !stats_ws_dev)
    return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  const uintptr_t esz = dtype == EULER_GPU_F32 ? 4 : 2, gsz = grad_dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)mask_dev % 8 != 0 || (uintptr_t)mask_t_dev % 8 != 0 || (uintptr_t)z_dev % esz != 0 ||
      (uintptr_t)root_dev % esz != 0 || (uintptr_t)s_src_dev % 4 != 0 || (uintptr_t)s_nb_dev % 4 != 0 ||
      (uintptr_t)s_root_dev % 4 != 0 || (uintptr_t)out_dev % gsz != 0 || (uintptr_t)grad_dev % gsz != 0 ||
      (uintptr_t)stats_ws_dev % 4 != 0 || (uintptr_t)d_z_dev % esz != 0 || (uintptr_t)d_root_dev % esz != 0 ||
      (uintptr_t)d_s_src_dev % 4 != 0 || (uintptr_t)d_s_nb_dev % 4 != 0 || (uintptr_t)d_s_root_dev % 4 != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  const bool f32 = dtype == EULER_GPU_F32;
  MaskAttBwdArgs a{};
  MaskAttArgs& f = a.f;
  f.mask = mask_dev; f.z = z_dev; f.s_src = s_src_dev; f.s_nb = s_nb_dev; f.root = root_dev; f.s_root = s_root_dev;
  f.out = const_cast<void*>(out_dev); f.batch = batch; f.n = (int32_t)n; f.m = (int32_t)m; f.d = (int32_t)d;
  f.heads = (int32_t)heads; f.dh = (int32_t)(d / heads); f.relu = activation == kMaskAttRelu;
  f.out_f32 = grad_dtype == EULER_GPU_F32; f.words = (int32_t)((m + 63) / 64); f.slope = negative_slope;
  f.plan = MaskAttBwdMakePlan(m, f.dh, f32, 1);
  f.waves = MaskWaves(batch, n, f.heads);
  a.grad = grad_dev; a.stats = stats_ws_dev; a.d_s_src = d_s_src_dev; a.d_s_root = d_s_root_dev; a.d_root = d_root_dev;
  a.mask_t = mask_t_dev; a.d_z = d_z_dev; a.d_s_nb = d_s_nb_dev; a.words_t = (int32_t)((n + 63) / 64);
  a.plan_t = MaskAttBwdMakePlan(n, f.dh, f32, 3);
  a.waves_t = MaskWaves(batch, m, f.heads);
  const bool vec_z = PoolVectorLoads(f.dh, (uintptr_t)z_dev, f32);
  // (an fp32 grad beside 16-bit z is loaded in two 16-byte halves of a piece of 8 columns: the 16-bit rule holds for both)
  const bool vec_g = PoolVectorLoads(f.dh, (uintptr_t)grad_dev, f32) && (!f.relu || (uintptr_t)out_dev % 16 == 0);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EULER_GPU_F32) return BwdDispatchTile<kF32>(st, a, vec_z, vec_g, candidates);
  if (dtype == EULER_GPU_BF16) return BwdDispatchTile<kBF16>(st, a, vec_z, vec_g, candidates);
  return BwdDispatchTile<kF16>(st, a, vec_z, vec_g, candidates);
}
