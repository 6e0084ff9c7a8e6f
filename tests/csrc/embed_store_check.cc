// Host build of the shared pieces of the in-place embedding stores (euler_amd/csrc/embed_store.h)
// for tests/test_embed_store_host.py: the range rule and the keys, the occurrence-to-source-row
// mapping, head / tail selection over the stably sorted (key, position) array, the add step and
// the single rounding - driven over whole calls on plain host arrays, one column at a time.
// Built with -ffp-contract=off.
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "embed_store.h"

using namespace euler_gpu;

namespace {

struct Call {
  void* table; int64_t rows, d;
  const int64_t* ids; int64_t e;
  const void* values; int64_t m; const int32_t* row_index; int64_t count;
  void* out; int32_t clear;
};

template <int DT>
uint32_t Get(const void* base, int64_t at) {
  if (DT == kF32) return static_cast<const uint32_t*>(base)[at];
  return static_cast<const uint16_t*>(base)[at];
}
template <int DT>
void Put(void* base, int64_t at, uint32_t raw) {
  if (DT == kF32) static_cast<uint32_t*>(base)[at] = raw;
  else static_cast<uint16_t*>(base)[at] = (uint16_t)raw;
}

// the stable sort of (key, position): what the radix sort of the device leaves
void Group(const Call& c, std::vector<uint64_t>* keys, std::vector<uint32_t>* perm) {
  std::vector<uint64_t> k((size_t)c.e);
  for (int64_t p = 0; p < c.e; ++p) k[p] = EsKey(c.ids[p], c.rows, EsSourceLive(p, c.row_index, c.m));
  perm->resize((size_t)c.e);
  std::iota(perm->begin(), perm->end(), 0u);
  std::stable_sort(perm->begin(), perm->end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
  keys->resize((size_t)c.e);
  for (int64_t i = 0; i < c.e; ++i) (*keys)[i] = k[(*perm)[i]];
}

template <int OP, int DT, int DV>
void Run(const Call& c) {
  if (OP == kEsTake) {
    for (int64_t p = 0; p < c.e; ++p)
      for (int64_t col = 0; col < c.d; ++col)
        Put<DV>(c.out, p * c.d + col,
                EsInRange(c.ids[p], c.rows) ? EsConvert<DT, DV>(Get<DT>(c.table, c.ids[p] * c.d + col)) : 0u);
    return;
  }
  std::vector<uint64_t> keys;
  std::vector<uint32_t> perm;
  Group(c, &keys, &perm);
  for (int64_t i = 0; i < c.e; ++i) {
    const bool live = keys[i] < (uint64_t)c.rows;
    const int64_t row = (int64_t)keys[i];
    if (OP == kEsUpdate) {
      if (!live || !EsIsTail(keys.data(), i, c.e)) continue;
      const int64_t src = EsSourceRow(perm[i], c.row_index, c.count);
      for (int64_t col = 0; col < c.d; ++col)
        Put<DT>(c.table, row * c.d + col, EsConvert<DV, DT>(Get<DV>(c.values, src * c.d + col)));
    } else if (OP == kEsAdd) {
      if (!live || !EsIsHead(keys.data(), i)) continue;
      for (int64_t col = 0; col < c.d; ++col) {
        float acc = EsWiden<DT>(Get<DT>(c.table, row * c.d + col));
        for (int64_t q = i; q < c.e && keys[q] == keys[i]; ++q)
          acc = EsAddStep<DV>(acc, Get<DV>(c.values, EsSourceRow(perm[q], c.row_index, c.count) * c.d + col));
        Put<DT>(c.table, row * c.d + col, EsNarrow<DT>(acc));
      }
    } else {                                      // kEsTakeClear
      if (!live) {
        for (int64_t col = 0; col < c.d; ++col) Put<DV>(c.out, (int64_t)perm[i] * c.d + col, 0u);
        continue;
      }
      if (!EsIsHead(keys.data(), i)) continue;
      for (int64_t col = 0; col < c.d; ++col) {
        const uint32_t old = EsConvert<DT, DV>(Get<DT>(c.table, row * c.d + col));
        for (int64_t q = i; q < c.e && keys[q] == keys[i]; ++q) Put<DV>(c.out, (int64_t)perm[q] * c.d + col, old);
        if (c.clear) Put<DT>(c.table, row * c.d + col, 0u);
      }
    }
  }
}

template <int OP, int DT>
void RunOther(const Call& c, int32_t other_dt) {
  if (other_dt == kF32) Run<OP, DT, kF32>(c);
  else Run<OP, DT, DT>(c);
}

template <int OP>
void RunTable(const Call& c, int32_t table_dt, int32_t other_dt) {
  if (table_dt == kF32) Run<OP, kF32, kF32>(c);
  else if (table_dt == kBF16) RunOther<OP, kBF16>(c, other_dt);
  else RunOther<OP, kF16>(c, other_dt);
}

}  // namespace

extern "C" int es_key_bits(int64_t rows) { return EsKeyBits(rows); }

extern "C" int es_chunk_width(int64_t d, uint64_t table, int table_bytes, uint64_t other, int other_bytes) {
  return EsChunkWidth(d, (uintptr_t)table, table_bytes, (uintptr_t)other, other_bytes);
}

// One whole call on host arrays.  op: 0 update, 1 add, 2 take (clear as given).  other / other_dt:
// values (update, add) or out (take); dtype codes 0 fp32, 1 bf16, 2 fp16 (16-bit data: uint16).
extern "C" int es_call(int32_t op, void* table, int32_t table_dt, int64_t rows, int64_t d, const int64_t* ids,
                       int64_t e, void* other, int32_t other_dt, int64_t m, const int32_t* row_index,
                       int64_t count, int32_t clear) {
  if (op < 0 || op > 2 || table_dt < 0 || table_dt > 2 || (other_dt != kF32 && other_dt != table_dt)) return -1;
  if (rows < 1 || e < 0 || d < 0 || (row_index && count != 0) || count < 0) return -1;
  if (op != 2 && count > 0 && (e % count != 0 || m != e / count)) return -1;
  if (op != 2 && !row_index && count == 0 && m != e) return -1;
  Call c{table, rows, d, ids, e, other, m, row_index, count, other, clear};
  if (op == 0) RunTable<kEsUpdate>(c, table_dt, other_dt);
  else if (op == 1) RunTable<kEsAdd>(c, table_dt, other_dt);
  else if (clear) RunTable<kEsTakeClear>(c, table_dt, other_dt);
  else RunTable<kEsTake>(c, table_dt, other_dt);
  return 0;
}
