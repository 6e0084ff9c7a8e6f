// The draw of Graph::SampleNode (core/graph/graph.cc:221-275) over the alias tables of a
// NodeSamplerView, shared by SampleNodeKernel (walk_kernels.hip) and SampleEdgeKernel
// (edge_kernels.hip): the reference's SampleNode and SampleEdge draw from one generator in the
// same program order, so both kernels consume exactly the same draws (domain NODE, stream 0).
#pragma once

#include "device_fns.h"

namespace euler_gpu {

struct SampleNodeArgs {
  NodeSamplerView s;
  uint64_t seed;
  uint64_t* out;
  uint32_t call_id;
  int32_t count;
  int32_t mode;          // 0 fixed type, 1 all types (-1), 2 type list
  int32_t type;          // mode 0
  int32_t n_sub;         // mode 2
  int32_t sub_type[kMaxNodeTypes];
  float sub_sum[kMaxNodeTypes];
};

__device__ __forceinline__ uint64_t AliasNext(const AliasEntry* tab, int64_t n,
                                              double u_col, double u_coin) {
  // AliasMethod::Next (alias_method.cc:66-78)
  const int64_t column = (int64_t)floor(__dmul_rn((double)n, u_col));
  const AliasEntry e = tab[column];
  return u_coin < (double)e.prob ? e.id_self : e.id_alias;
}

// Sample i of a call: the id of the alias entry it draws.
__device__ __forceinline__ uint64_t SampleNodeDraw(const SampleNodeArgs& a, int64_t i) {
  int32_t t = a.type;
  uint64_t d = 0;   // index of the next draw of this sample
  if (a.mode == 0) {
    d = 2 * (uint64_t)i;
  } else if (a.mode == 1) {
    d = 4 * (uint64_t)i;
    const Philox4 b = RngBlock(a.seed, a.call_id, kDomainNode, 0,
                               (uint32_t)(d >> 1));
    const int64_t col = (int64_t)floor(__dmul_rn(
        (double)a.s.n_types, UnitFromWords(b.w[0], b.w[1])));
    t = UnitFromWords(b.w[2], b.w[3]) < (double)a.s.tc_prob[col]
            ? (int32_t)col : a.s.tc_alias[col];
    d += 2;
  } else {
    d = 3 * (uint64_t)i;
    const double u = RngDraw(a.seed, a.call_id, kDomainNode, 0, d);
    t = a.sub_type[RandomSelect(a.sub_sum, 0, (uint64_t)(a.n_sub - 1), u)];
    d += 1;
  }
  const double u_col = RngDraw(a.seed, a.call_id, kDomainNode, 0, d);
  const double u_coin = RngDraw(a.seed, a.call_id, kDomainNode, 0, d + 1);
  const int64_t b = a.s.type_off[t];
  return AliasNext(a.s.entries + b, a.s.type_off[t + 1] - b, u_col, u_coin);
}

// The host half of Graph::SampleNode: the mode and type list of a call (api.cc:33-35,
// graph.cc:229-275).  `what` prefixes the error messages, `noun` names the records.
inline int PrepareSampleNode(const NodeSamplerView& s, const int32_t* types_host, int32_t k,
                             const char* what, const char* noun, SampleNodeArgs* a) {
  const int32_t T = s.n_types;
  if (k == 1) {
    const int32_t type = types_host[0];
    if (type == -1) {
      if (s.tc_sum == 0.f)
        return Fail(EULER_GPU_EEMPTY, std::string(what) + ": total " + noun + " weight is 0");
      a->mode = 1;
    } else {
      if (type < 0 || type >= T)
        return Fail(EULER_GPU_EINVAL, std::string(what) + ": " + noun + " type out of range");
      if (s.sampler_sum[type] == 0.f || s.type_off[type + 1] == s.type_off[type])
        return Fail(EULER_GPU_EEMPTY, std::string(what) + ": type weight is 0");
      a->mode = 0; a->type = type;
    }
    return EULER_GPU_OK;
  }
  a->mode = 2;
  float acc = 0.f;
  int32_t m = 0;
  for (int32_t t = 0; t < T; ++t) {
    bool in = false;
    for (int32_t j = 0; j < k; ++j) in |= types_host[j] == t;
    if (in) {
      acc += s.type_sum[t];
      a->sub_type[m] = t; a->sub_sum[m] = acc; ++m;
    }
  }
  a->n_sub = m;
  if (m == 0 || !(a->sub_sum[m - 1] > 0.f))
    return Fail(EULER_GPU_EEMPTY, std::string(what) + ": listed types have zero weight");
  return EULER_GPU_OK;
}

}  // namespace euler_gpu
