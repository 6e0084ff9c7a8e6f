// The all-or-none rule of the op kernels (euler_amd/csrc/op_framework.cc: OpOutputs), driven without
// any device error: OpKernelContext::Allocate / AddAlias fail when the name exists, so a caller that
// pre-allocates one of an op's output names sends the op through its rollback.  After every failing
// run: none of the names the op created is left, the caller's tensor is the same Tensor* with the
// same bytes, the inputs are intact - and the same op in a fresh context succeeds with all outputs.
//   op_rollback_check        every case (needs a GPU)
//   op_rollback_check host   the host-only ops; without a device also: ID_UNIQUE leaves no output
// Exits 1 with a message on the first violated check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "euler_gpu.h"
#include "euler_op_framework.h"

using namespace euler;

#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "FAIL %s:%d (%s): ", __FILE__, __LINE__, #cond);     \
      fprintf(stderr, __VA_ARGS__);                                        \
      fprintf(stderr, "\n");                                               \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

static euler_gpu_graph* g_graph = nullptr;
typedef std::function<void(OpKernelContext*)> Fill;

template <typename T>
static Tensor* Put(OpKernelContext* ctx, const std::string& name, DataType type, const std::vector<T>& v) {
  Tensor* t = nullptr;
  CHECK(ctx->Allocate(name, {v.size()}, type, &t) == 0, "input %s", name.c_str());
  if (!v.empty()) memcpy(t->Raw<T>(), v.data(), v.size() * sizeof(T));
  return t;
}

static Tensor* Get(OpKernelContext* ctx, const std::string& name) {
  Tensor* t = nullptr;
  return ctx->tensor(name, &t) == 0 ? t : nullptr;
}

static void Run(const NodeDef& nd, OpKernelContext* ctx) {
  OpKernel* k = nullptr;
  CHECK(CreateOpKernel(nd.op, &k) == 0, "no kernel %s", nd.op.c_str());
  ctx->SetGraph(g_graph);
  ctx->SetSeed(1);
  ctx->SetCallId(0);
  k->Compute(nd, ctx);
}

static void ExpectOutputs(const NodeDef& nd, OpKernelContext* ctx, int n_out, const char* what) {
  for (int i = 0; i < n_out; ++i)
    CHECK(Get(ctx, OutputName(nd, i)) != nullptr, "%s %s: output %d missing", nd.op.c_str(), what, i);
}

// The op with output `taken` already in the context (the caller's 3 bytes of 0x5A), then the op
// again in a fresh context.  `fill` allocates the inputs; `check` inspects the successful run.
static void Collide(const NodeDef& nd, const Fill& fill, int n_out, int taken,
                    const std::function<void(OpKernelContext*)>& check = nullptr) {
  {
    OpKernelContext ctx;
    fill(&ctx);
    struct Snap { std::string name; Tensor* t; std::string bytes; };
    std::vector<Snap> snaps;
    for (const std::string& in : nd.inputs)
      if (Tensor* t = Get(&ctx, in))
        if (t->Type() != kString) snaps.push_back({in, t, std::string(t->Raw<char>(), t->TotalBytes())});
    Tensor* mine = nullptr;
    CHECK(ctx.Allocate(OutputName(nd, taken), {3}, kUInt8, &mine) == 0, "pre-allocate");
    memset(mine->Raw<uint8_t>(), 0x5A, 3);
    Run(nd, &ctx);
    for (int i = 0; i < n_out + 2; ++i) {
      Tensor* t = Get(&ctx, OutputName(nd, i));
      if (i != taken) {
        CHECK(t == nullptr, "%s: output %d left behind (output %d was taken)", nd.op.c_str(), i, taken);
        continue;
      }
      CHECK(t == mine && t->Type() == kUInt8 && t->NumElements() == 3, "%s: the caller's tensor was replaced", nd.op.c_str());
      for (int b = 0; b < 3; ++b) CHECK(t->Raw<uint8_t>()[b] == 0x5A, "%s: the caller's tensor was written", nd.op.c_str());
    }
    for (const Snap& s : snaps) {
      Tensor* t = Get(&ctx, s.name);
      CHECK(t == s.t, "%s: input %s is gone", nd.op.c_str(), s.name.c_str());
      CHECK(std::string(t->Raw<char>(), t->TotalBytes()) == s.bytes, "%s: input %s changed", nd.op.c_str(), s.name.c_str());
    }
  }   // the context frees every tensor once
  OpKernelContext ctx;
  fill(&ctx);
  Run(nd, &ctx);
  ExpectOutputs(nd, &ctx, n_out, "after a failed run");
  if (check) check(&ctx);
}

static void CheckUnique(OpKernelContext* ctx, const NodeDef& nd, const std::vector<uint64_t>& ids, size_t n_unique) {
  Tensor *uq = Get(ctx, OutputName(nd, 0)), *gi = Get(ctx, OutputName(nd, 1));
  CHECK(uq != nullptr && gi != nullptr, "ID_UNIQUE: outputs missing");
  CHECK((size_t)uq->NumElements() == n_unique && (size_t)gi->NumElements() == ids.size(),
        "ID_UNIQUE: %d unique of %d", uq->NumElements(), gi->NumElements());
  for (size_t i = 0; i < ids.size(); ++i) {
    const int32_t r = gi->Raw<int32_t>()[i];
    CHECK(r >= 0 && (size_t)r < n_unique && uq->Raw<uint64_t>()[r] == ids[i], "ID_UNIQUE: uq[gi[%zu]] != ids[%zu]", i, i);
  }
}

static void HostOnlyCases() {
  // API_SPARSE_GEN_ADJ: roots [batch 2 x n 2], l_nb, n -> :0 (root, batch row) pairs, :1 an alias of l_nb
  const std::vector<uint64_t> roots = {11, 12, 13, 14}, l_nb = {21, 22, 23};
  NodeDef gen{"API_SPARSE_GEN_ADJ,0", "API_SPARSE_GEN_ADJ", {"roots", "l_nb", "n"}, {}};
  Collide(gen, [&](OpKernelContext* c) {
    Put(c, "roots", kUInt64, roots);
    Put(c, "l_nb", kUInt64, l_nb);
    Put(c, "n", kInt32, std::vector<int32_t>{2});
  }, 2, 1, [&](OpKernelContext* c) {
    Tensor* rb = Get(c, OutputName(gen, 0));
    CHECK(rb->NumElements() == 8, "API_SPARSE_GEN_ADJ: shape");
    for (int r = 0; r < 4; ++r)
      CHECK(rb->Raw<uint64_t>()[2 * r] == roots[r] && rb->Raw<uint64_t>()[2 * r + 1] == (uint64_t)(r / 2),
            "API_SPARSE_GEN_ADJ: row %d", r);
    CHECK(Get(c, OutputName(gen, 1)) == Get(c, "l_nb"), "API_SPARSE_GEN_ADJ: :1 is not l_nb");
  });
  // API_GATHER_RESULT: three aliases; output 2 taken, then the third input missing
  const Fill three = [&](OpKernelContext* c) {
    Put(c, "a", kInt32, std::vector<int32_t>{0, 1, 1, 3});
    Put(c, "b", kUInt64, std::vector<uint64_t>{5, 6, 7});
    Put(c, "c", kUInt64, l_nb);
  };
  NodeDef gather{"API_GATHER_RESULT,1", "API_GATHER_RESULT", {"a", "b", "c"}, {}};
  const auto aliases = [&](OpKernelContext* c) {
    for (int i = 0; i < 3; ++i)
      CHECK(Get(c, OutputName(gather, i)) == Get(c, gather.inputs[i]), "API_GATHER_RESULT: alias %d", i);
  };
  Collide(gather, three, 3, 2, aliases);
  {
    OpKernelContext ctx;
    three(&ctx);
    Tensor *a = Get(&ctx, "a"), *b = Get(&ctx, "b");
    NodeDef missing{"API_GATHER_RESULT,1", "API_GATHER_RESULT", {"a", "b", "nowhere"}, {}};
    Run(missing, &ctx);
    for (int i = 0; i < 3; ++i) CHECK(Get(&ctx, OutputName(missing, i)) == nullptr, "API_GATHER_RESULT: alias %d left behind", i);
    CHECK(Get(&ctx, "a") == a && Get(&ctx, "b") == b && a->Raw<int32_t>()[3] == 3 && b->Raw<uint64_t>()[2] == 7,
          "API_GATHER_RESULT: inputs damaged");
  }
  OpKernelContext ctx;
  three(&ctx);
  Run(gather, &ctx);
  aliases(&ctx);
}

static void DeviceCases() {
  const std::vector<int32_t> et = {0}, cnt = {3}, minus1 = {-1};
  const std::vector<uint64_t> nodes = {5, 17, 5, 200, 1};
  // ID_UNIQUE, no graph
  const std::vector<uint64_t> ids = {7, 3, 7, 9, 3};
  NodeDef uq{"ID_UNIQUE,0", "ID_UNIQUE", {"ids"}, {}};
  const Fill f_ids = [&](OpKernelContext* c) { Put(c, "ids", kUInt64, ids); };
  {
    OpKernelContext ctx;
    f_ids(&ctx);
    Run(uq, &ctx);
    CheckUnique(&ctx, uq, ids, 3);
  }
  Collide(uq, f_ids, 2, 1, [&](OpKernelContext* c) { CheckUnique(c, uq, ids, 3); });
  // 4 096 ids, 4 093 of them distinct: :0 is 32 KB and :1 16 KB, pinned blocks of the pool.  The block
  // of :0 goes back to the pool in the rollback (after the drain) and serves the second run.
  std::vector<uint64_t> many(4096);
  for (size_t i = 0; i < many.size(); ++i) many[i] = 1 + (i * 2654435761ull) % 4093;
  Collide(uq, [&](OpKernelContext* c) { Put(c, "ids", kUInt64, many); }, 2, 1,
          [&](OpKernelContext* c) { CheckUnique(c, uq, many, 4093); });
  // IDX_GATHER / DATA_GATHER: rows (0,2) (2,3) (3,5) gathered as 0 1 0 2 1
  const std::vector<int32_t> idx = {0, 2, 2, 3, 3, 5}, gi = {0, 1, 0, 2, 1};
  const std::vector<uint64_t> data = {10, 11, 12, 13, 14};
  const Fill f_gather = [&](OpKernelContext* c) {
    Put(c, "data", kUInt64, data);
    Put(c, "idx", kInt32, idx);
    Put(c, "gi", kInt32, gi);
  };
  NodeDef ig{"IDX_GATHER,1", "IDX_GATHER", {"idx", "gi"}, {}};
  Collide(ig, f_gather, 1, 0, [&](OpKernelContext* c) {
    const int32_t want[10] = {0, 2, 2, 3, 3, 5, 5, 7, 7, 8};
    Tensor* o = Get(c, OutputName(ig, 0));
    CHECK(o->NumElements() == 10 && memcmp(o->Raw<int32_t>(), want, sizeof(want)) == 0, "IDX_GATHER: result");
  });
  NodeDef dg{"DATA_GATHER,2", "DATA_GATHER", {"data", "idx", "gi"}, {}};
  Collide(dg, f_gather, 1, 0, [&](OpKernelContext* c) {
    const uint64_t want[8] = {10, 11, 12, 10, 11, 13, 14, 12};
    Tensor* o = Get(c, OutputName(dg, 0));
    CHECK(o->NumElements() == 8 && memcmp(o->Raw<uint64_t>(), want, sizeof(want)) == 0, "DATA_GATHER: result");
  });
  // the graph ops
  const Fill f_nodes = [&](OpKernelContext* c) {
    Put(c, "nodes", kUInt64, nodes);
    Put(c, "et", kInt32, et);
    Put(c, "count", kInt32, cnt);
    Put(c, "default_node", kInt32, minus1);
  };
  NodeDef nb{"API_GET_NB_NODE,3", "API_GET_NB_NODE", {"nodes", "et"}, {}};
  Collide(nb, f_nodes, 4, 3, [&](OpKernelContext* c) {
    Tensor *o_idx = Get(c, OutputName(nb, 0)), *o_id = Get(c, OutputName(nb, 1));
    CHECK(o_idx->NumElements() == 10 && o_idx->Raw<int32_t>()[9] == o_id->NumElements(), "API_GET_NB_NODE: idx");
    for (int i = 0; i < 5; ++i)
      CHECK(o_idx->Raw<int32_t>()[2 * i + 1] > o_idx->Raw<int32_t>()[2 * i], "API_GET_NB_NODE: node %d has no neighbour", i);
  });
  NodeDef snb{"API_SAMPLE_NB,4", "API_SAMPLE_NB", {"nodes", "et", "count", "default_node"}, {}};
  Collide(snb, f_nodes, 4, 2, [&](OpKernelContext* c) {
    CHECK(Get(c, OutputName(snb, 1))->NumElements() == 15, "API_SAMPLE_NB: 5 x 3 samples");
  });
  snb.post_process = {"order_by id", "limit 2"};
  Collide(snb, f_nodes, 4, 2, [&](OpKernelContext* c) {
    Tensor *o_idx = Get(c, OutputName(snb, 0)), *o_id = Get(c, OutputName(snb, 1));
    CHECK(o_id->NumElements() == 10, "API_SAMPLE_NB limit 2: %d entries", o_id->NumElements());
    for (int i = 0; i < 5; ++i) {
      const int32_t b = o_idx->Raw<int32_t>()[2 * i];
      CHECK(o_idx->Raw<int32_t>()[2 * i + 1] == b + 2 && o_id->Raw<uint64_t>()[b] <= o_id->Raw<uint64_t>()[b + 1],
            "API_SAMPLE_NB order_by id; limit 2: row %d", i);
    }
  });
  NodeDef sw{"API_GET_EDGE_SUM_WEIGHT,5", "API_GET_EDGE_SUM_WEIGHT", {"nodes", "et"}, {}};
  Collide(sw, f_nodes, 2, 1, [&](OpKernelContext* c) {
    Tensor *r = Get(c, OutputName(sw, 0)), *w = Get(c, OutputName(sw, 1));
    for (int i = 0; i < 5; ++i)
      CHECK(r->Raw<uint64_t>()[i] == nodes[i] && w->Raw<float>()[i] > 0.f, "API_GET_EDGE_SUM_WEIGHT: row %d", i);
  });
  NodeDef sl{"API_SAMPLE_L,6", "API_SAMPLE_L", {"nodes", "et", "-1"}, {}};
  Collide(sl, f_nodes, 3, 2, [&](OpKernelContext* c) {
    CHECK(Get(c, OutputName(sl, 0))->NumElements() == 5, "API_SAMPLE_L: one draw per root");
  });
}

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && strcmp(argv[1], "host") == 0;
  HostOnlyCases();
  if (host_only) {
    if (euler_gpu_device_count() > 0) { printf("host-only ops ok\n"); return 0; }
    // no device: a device op logs and leaves no output
    OpKernelContext ctx;
    Put(&ctx, "ids", kUInt64, std::vector<uint64_t>{7, 3, 7, 9, 3});
    NodeDef uq{"ID_UNIQUE,0", "ID_UNIQUE", {"ids"}, {}};
    Run(uq, &ctx);
    CHECK(Get(&ctx, OutputName(uq, 0)) == nullptr && Get(&ctx, OutputName(uq, 1)) == nullptr,
          "ID_UNIQUE without a device left an output");
    printf("host-only ops ok; no device: ID_UNIQUE left no output\n");
    return 0;
  }
  euler_gpu_synth_params p{};
  p.seed = 7; p.n_nodes = 300; p.n_edges_target = 3000; p.n_types = 1; p.weighted = 1;
  p.scale = 9;                                              // 2^9 >= 300
  for (int z = 0; z < 64; ++z) p.deg_table[z] = 9.0;        // min degree 1: every node has a neighbour
  if (euler_gpu_graph_create_synthetic(&p, 0, 1, 0, 1, &g_graph) != 0) {
    fprintf(stderr, "graph: %s\n", euler_gpu_last_error());
    return 1;
  }
  DeviceCases();
  euler_gpu_graph_destroy(g_graph);
  printf("all ops ok\n");
  return 0;
}
