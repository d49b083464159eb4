// tie_tables.hip -- option "tie_rule" on the host: the order tables of the reference's kd-trees (target points, target features, transformed
// source), when they are built or loaded, and the cilhip_*tie* entry points.  The tables themselves are built on the device (tie_build.hip).
#include <algorithm>
#include <chrono>
#include <cstring>

#include "ctx.hpp"

// ---- option "tie_rule": the reference's order among exactly equidistant nearest points ------------------------------------------
// When the option is in force for a context's searches: the order is the reference's kd-tree over the TARGET POINTS: it covers the
// SECOND_TO_FIRST matches (also the forward half of BOTH) under rigid and affine transforms.  Feature adaptors search another
// space (nanoflann's DIM = 6 / 9 tree: tie_feat_on below), the reverse matches of FIRST_TO_SECOND / BOTH a tree over the transformed
// SOURCE that the reference rebuilds every iteration (rev_tie_aware); the feature adaptors' reverse searches keep the lowest index
// (tie_rule 2) or are refused (tie_rule 1, the explicit request).  An
// index shard of a target (cilhip_set_shard_info) notices and counts ties like any context, but never builds tables from its own points:
// the order belongs to the WHOLE target's tree -- whoever owns the shards loads it (cilhip_load_tie_order with the global indices) and
// runs the two-key protocol between them (cilhip_icp_order_keys).  (The predicate itself: tie_mode_on, ctx.hpp.)
// ... and over 6-D / 9-D features: the forward (SECOND_TO_FIRST) search of a whole target follows the reference's DIM = 6 / 9 tree
// (its order tables: tie_order_build_device_features; tie_settle<true> / tie_before_nd on the device)
static bool tie_feat_on(const cilhip_ctx* c) { return c->tie_rule != 0 && feat6(c) && c->search_dir == 0 && !c->partial_target && !c->index_offset; }
TieDev cilhip::tie_dev_of(const cilhip_ctx* c) {
  TieDev t{};
  if (feat6(c)) {
    t.mode = tie_feat_on(c) ? 1 : 0;
    t.leaf_slot = t.mode ? c->d_tief_leaf_slot : nullptr;
    t.nodes = c->d_tief_nodes;
    t.counters = c->d_tie_counters;
    return t;
  }
  t.mode = tie_mode_on(c) ? 1 : 0;
  t.leaf_slot = t.mode ? c->d_tie_leaf_slot : nullptr;
  t.nodes = c->d_tie_nodes;
  t.counters = c->d_tie_counters;
  return t;
}
// Order tables by this target's ORIGINAL (local) index -> device, by sorted position.
static int load_tie_tables(cilhip_ctx* c, const uint32_t* leaf_by_index, const uint32_t* slot_by_index, const cilhip::TieNode* nodes, size_t n_nodes) {
  static_assert(sizeof(cilhip::TieNode) == sizeof(uint4), "TieNode is read as one 16-byte record");
  CK(c, hipSetDevice(c->device));
  drop_tie_tables(c);
  const size_t n = c->grid.n;
  DevBuf<uint32_t> d_leaf, d_slot;
  // (d_tie_leaf_slot != null is the "tables loaded" flag: nothing may be left half set when an allocation fails)
  hipError_t e = c->d_tie_leaf_slot.alloc(n);
  if (e == hipSuccess) e = c->d_tie_nodes.alloc(n_nodes);
  if (e == hipSuccess) e = d_leaf.alloc(n);
  if (e == hipSuccess) e = d_slot.alloc(n);
  if (e == hipSuccess && n) {
    e = hipMemcpyAsync(d_leaf, leaf_by_index, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_slot, slot_by_index, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n_nodes) e = hipMemcpyAsync(c->d_tie_nodes, nodes, n_nodes * sizeof(uint4), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_tie_tables_by_position(c->grid.pts, c->grid.n, d_leaf, d_slot, c->d_tie_leaf_slot, c->stream); e = hipGetLastError(); }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // (the host arrays and the two staging buffers live on this frame)
  if (e != hipSuccess) { drop_tie_tables(c); c->err = std::string("tie_rule: loading the order tables: ") + hipGetErrorString(e); return CILHIP_ERR_HIP; }
  for (size_t k = 0; k < n_nodes; ++k) c->tie_max_depth = std::max(c->tie_max_depth, (int)(nodes[k].info >> 3));
  return CILHIP_OK;
}
// The order tables of a tree over this context's target, built on the device (tie_build.hip): `build` fills leaf and slot by original
// index and the nodes; the tables by sorted position go to *leaf_slot.  On failure the caller drops what *leaf_slot holds.
template <class Build>
static hipError_t build_target_order_tables(cilhip_ctx* c, SharedBuf<uint2>& leaf_slot, SharedBuf<uint4>& nodes, Build build) {
  const uint32_t n = c->grid.n;
  DevBuf<uint32_t> d_leaf, d_slot;
  DevBuf<uint4> d_nodes;
  hipError_t e = d_leaf.alloc(n);
  if (e == hipSuccess) e = d_slot.alloc(n);
  if (e == hipSuccess) e = leaf_slot.alloc(n);
  if (e == hipSuccess) e = build(d_leaf.get(), d_slot.get(), &d_nodes);
  if (e == hipSuccess && !d_nodes) e = d_nodes.alloc(1);      // (an empty target)
  if (e == hipSuccess && n) { launch_tie_tables_by_position(c->grid.pts, n, d_leaf, d_slot, leaf_slot, c->stream); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = nodes.adopt(std::move(d_nodes));
  return e;
}
// The tables of THIS context's target, from the grid's own records.
int cilhip::build_tie_tables(cilhip_ctx* c) {
  if (c->d_tie_leaf_slot || !c->has_target) return CILHIP_OK;
  const auto t0 = std::chrono::steady_clock::now();
  CK(c, hipSetDevice(c->device));
  drop_tie_tables(c);
  size_t n_nodes = 0;
  int depth = 0;
  const hipError_t e = build_target_order_tables(c, c->d_tie_leaf_slot, c->d_tie_nodes, [&](uint32_t* leaf, uint32_t* slot, DevBuf<uint4>* nodes) {
    return tie_order_build_device(nullptr, c->grid.pts, c->grid.n, c->stream, leaf, slot, nodes, &n_nodes, &depth); });
  if (e != hipSuccess) {
    drop_tie_tables(c);
    c->err = std::string("tie_rule: building the order tables: ") + hipGetErrorString(e);
    return CILHIP_ERR_HIP;
  }
  c->tie_max_depth = depth;
  c->tie_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  ++c->tie_builds;
  return CILHIP_OK;
}
// the counters of the searches since the last launch_init_state (a host round trip)
static int read_tie_counters(cilhip_ctx* c, unsigned int out[4]) {
  CK(c, hipMemcpyAsync(out, c->d_tie_counters, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return CILHIP_OK;
}
// The reverse matches' order (FIRST_TO_SECOND / BOTH): what k_reverse_search is handed.  Without valid tables it counts the tied target
// points (counters[3]) and keeps the lowest source index.
TieDev cilhip::tie_dev_rev(const cilhip_ctx* c) {
  TieDev t{};
  t.mode = tie_mode_on(c) ? 1 : 0;
  t.leaf_slot = (t.mode && c->rev_tie_valid) ? c->d_rev_tie_leaf_slot : nullptr;
  t.nodes = c->d_rev_tie_nodes;
  t.counters = c->d_tie_counters;
  return t;
}
// The order tables of the tree the reference builds over the source transformed by T (src_points_trans = transform_ * src, the engine's
// pinned f32 expression; correspondence_search_kd_tree.hpp:185-222), by position in the source grid.  Device work per search: the
// transform of the source (its original order) and tie_order_build_device over it (2 ms for a 110k-point frame, 25 ms at 10M).
int cilhip::build_rev_tie_tables(cilhip_ctx* c, const float T[16]) {
  if (c->rev_tie_valid && memcmp(c->rev_tie_T, T, sizeof(c->rev_tie_T)) == 0) return CILHIP_OK;
  c->rev_tie_valid = false;
  const uint32_t n = c->ns;
  if (!c->has_src_grid || n == 0) return CILHIP_OK;
  CK(c, hipSetDevice(c->device));
  DevBuf<float> d_q;
  DevBuf<uint32_t> d_leaf, d_slot;
  DevBuf<uint4> d_nodes;
  size_t n_nodes = 0;
  hipError_t e = d_q.alloc((size_t)n * 3);
  if (e == hipSuccess) e = d_leaf.alloc(n);
  if (e == hipSuccess) e = d_slot.alloc(n);
  if (e == hipSuccess && !c->d_rev_tie_leaf_slot) e = c->d_rev_tie_leaf_slot.alloc(n);
  if (e == hipSuccess) { launch_transform_original_host_T(c->d_src_xyz, n, T, d_q, c->stream); e = hipGetLastError(); }      // q = fl(T s), the engine's pinned expression
  if (e == hipSuccess) e = tie_order_build_device(d_q, nullptr, n, c->stream, d_leaf, d_slot, &d_nodes, &n_nodes, nullptr);
  if (e == hipSuccess) {
    c->d_rev_tie_nodes = std::move(d_nodes);
    launch_tie_tables_by_position(c->src_grid.pts, n, d_leaf, d_slot, c->d_rev_tie_leaf_slot, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { c->err = std::string("tie_rule: the transformed source's order tables: ") + hipGetErrorString(e); return CILHIP_ERR_HIP; }
  memcpy(c->rev_tie_T, T, sizeof(c->rev_tie_T));
  c->rev_tie_valid = true;
  ++c->rev_tie_builds;
  return CILHIP_OK;
}
// tie_rule 1: the tables before the first search; refusals of the explicit request (see tie_mode_on)
// The order tables of the tree the reference's feature adaptor searches (DIM = 6: points + weighted normals or colours; 9: + colours), for
// this target under the CURRENT feature options, built on the device (tie_build.hip).
static int build_feat_tie_tables(cilhip_ctx* c) {
  if (c->d_tief_leaf_slot || !c->has_target) return CILHIP_OK;
  CK(c, hipSetDevice(c->device));
  { const int rc = ensure_feature_arrays(c); if (rc) return rc; }
  const FeatSpec f = feat_spec_of(c);
  const int dim = c->feature_kind == 2 ? 9 : 6;
  if (!f.dst || (dim == 9 && !f.dst2)) return fail(c, CILHIP_ERR_INVALID, "tie_rule: the target's feature attributes (normals / colours) are not set");
  size_t n_nodes = 0;
  const hipError_t e = build_target_order_tables(c, c->d_tief_leaf_slot, c->d_tief_nodes, [&](uint32_t* leaf, uint32_t* slot, DevBuf<uint4>* nodes) {
    return tie_order_build_device_features(dim, c->grid.pts, f.dst, f.w, f.dst2, f.w2, c->grid.n, c->stream, leaf, slot, nodes, &n_nodes, nullptr); });
  if (e != hipSuccess) {
    drop_feat_tie_tables(c);
    c->err = std::string("tie_rule: building the feature tree's order tables: ") + hipGetErrorString(e);
    return CILHIP_ERR_HIP;
  }
  ++c->tief_builds;
  return CILHIP_OK;
}
int cilhip::tie_prepare(cilhip_ctx* c, const char* what) {
  c->tie_counters_fresh = false;      // (a new search / run: whatever the host holds of the counters is history)
  if (c->tie_rule == 1 && ((feat6(c) && !tie_feat_on(c)) || (!feat6(c) && c->partial_target && !c->d_tie_leaf_slot))) {
    c->err = std::string(what) + ": tie_rule = 1 covers the SECOND_TO_FIRST search (point features: every direction) on a whole target, or on shards of a point-feature target with the whole target's order loaded (tie_rule = 2 applies the reference's order where it is defined)";
    return CILHIP_ERR_UNSUPPORTED;
  }
  if (c->tie_rule == 1 && tie_feat_on(c) && c->ns && c->grid.n) return build_feat_tie_tables(c);
  if (c->tie_rule == 1 && c->search_dir != 0) c->rev_tie_aware = true;
  if (c->tie_rule == 0) c->rev_tie_aware = false;
  if (c->tie_rule == 1 && tie_mode_on(c) && !c->partial_target && c->search_dir != 1 && c->ns && c->grid.n) return build_tie_tables(c);
  return CILHIP_OK;
}
// After a search / run: did it meet ties without tables (tie_rule 2)?  Then the tables are built and *again says: run it once more.
int cilhip::tie_check_pending(cilhip_ctx* c, bool* again) {
  *again = false;
  if (tie_feat_on(c)) {      // a feature search: its forward matches counted tied queries while the feature tree's tables were not there
    if (c->d_tief_leaf_slot || !c->ns || !c->grid.n) return CILHIP_OK;
    unsigned int cnt[4];
    if (c->tie_counters_fresh) memcpy(cnt, c->tie_counters_host, sizeof(cnt));
    else { const int rc = read_tie_counters(c, cnt); if (rc) return rc; }
    c->tie_counters_fresh = false;
    if (cnt[0] == 0u) return CILHIP_OK;
    *again = true;
    CK(c, hipMemsetAsync(c->d_tie_counters, 0, 4 * sizeof(unsigned int), c->stream));
    return build_feat_tie_tables(c);
  }
  if (!tie_mode_on(c) || c->partial_target || !c->ns || !c->grid.n) return CILHIP_OK;      // (a part of a target: its caller loads the whole cloud's order)
  const bool fwd_open = !c->d_tie_leaf_slot && c->search_dir != 1;      // (forward matches: SECOND_TO_FIRST, the forward half of BOTH)
  const bool rev_open = !c->rev_tie_aware && c->search_dir != 0;
  if (!fwd_open && !rev_open) return CILHIP_OK;
  unsigned int cnt[4];
  if (c->tie_counters_fresh) {      // (a run's read_state has just brought them over with the loop state: no second round trip)
    memcpy(cnt, c->tie_counters_host, sizeof(cnt));
  } else {
    const int rc = read_tie_counters(c, cnt);
    if (rc) return rc;
  }
  c->tie_counters_fresh = false;
  // Forward matches: any tie, the tables are built once per target.  Reverse matches: the tables cost a host tree build PER SEARCH (0.25 s
  // at 10M points against an iteration of a millisecond), so the automatic rule pays it for clouds that tie systematically -- duplicated
  // points, lattices: at least 16 tied target points and one in 100 000 -- and not for the isolated coincidence of two f32 distances in a
  // large random cloud (about one target point in ten million): those keep the lowest source index and stay counted
  // (cilhip_get_tie_rule_stats); tie_rule 1 follows the reference for every one of them.
  const bool fwd = fwd_open && cnt[0] != 0u, rev = rev_open && cnt[3] >= 16u && (unsigned long long)cnt[3] * 100000ull >= (unsigned long long)c->grid.n;
  if (!fwd && !rev) return CILHIP_OK;
  *again = true;
  CK(c, hipMemsetAsync(c->d_tie_counters, 0, 4 * sizeof(unsigned int), c->stream));      // (the repeated search counts afresh)
  if (rev) c->rev_tie_aware = true;      // (the tables themselves: per search, under its transform -- run_pair_search)
  return fwd ? build_tie_tables(c) : CILHIP_OK;
}

int cilhip_get_tie_count(cilhip_ctx* c, const float T[16], float max_sq, size_t* n_ties) {
  if (!c || !T || !n_ties) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  const int rc = ensure_sorted(c, T);
  if (rc) return rc;
  launch_count_ties(c->grid, c->d_src_sorted, c->ns, T, max_sq, c->d_count, c->stream);
  unsigned long long v = 0;
  CK(c, hipMemcpyAsync(&v, c->d_count, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  CK(c, hipGetLastError());
  *n_ties = (size_t)v;
  return CILHIP_OK;
}

struct cilhip_tie_order { std::vector<uint32_t> leaf, slot; std::vector<cilhip::TieNode> nodes; uint32_t n = 0; int max_depth = 0; };
int cilhip_tie_order_create(const float* xyz, size_t n, cilhip_tie_order** out) {
  if (!out || (n && !xyz) || n >= 0xFFFFFFF0ull) return CILHIP_ERR_INVALID;
  *out = nullptr;
  int ndev = 0, dev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CILHIP_ERR_NO_DEVICE;      // (built on the device: no CPU fallback)
  cilhip_tie_order* o = nullptr;
  DevBuf<float> d_xyz;
  DevBuf<uint32_t> d_leaf, d_slot;
  DevBuf<uint4> d_nodes;
  size_t n_nodes = 0;
  StreamGuard s;      // (declared last: drained and destroyed before the buffers go)
  hipError_t e = hipSuccess;
  int rc = CILHIP_OK;
  try {
    o = new cilhip_tie_order();
    o->n = (uint32_t)n;
    o->leaf.assign(n, 0u); o->slot.assign(n, 0u);
    if (n) {
      e = s.create();
      if (e == hipSuccess) e = d_xyz.alloc(n * 3);
      if (e == hipSuccess) e = d_leaf.alloc(n);
      if (e == hipSuccess) e = d_slot.alloc(n);
      if (e == hipSuccess) e = hipMemcpyAsync(d_xyz, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = tie_order_build_device(d_xyz, nullptr, (uint32_t)n, s, d_leaf, d_slot, &d_nodes, &n_nodes, &o->max_depth);
      if (e == hipSuccess) { o->nodes.resize(n_nodes); e = hipMemcpyAsync(o->nodes.data(), d_nodes, n_nodes * sizeof(uint4), hipMemcpyDeviceToHost, s); }
      if (e == hipSuccess) e = hipMemcpyAsync(o->leaf.data(), d_leaf, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipMemcpyAsync(o->slot.data(), d_slot, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
  } catch (...) { rc = CILHIP_ERR_HIP; }      // (out of host memory: never across the C boundary)
  if (e != hipSuccess) rc = CILHIP_ERR_HIP;
  if (rc != CILHIP_OK) { delete o; return rc; }
  *out = o;
  return CILHIP_OK;
}
void cilhip_tie_order_destroy(cilhip_tie_order* order) { delete order; }
int cilhip_tie_order_tables(const cilhip_tie_order* o, uint32_t* leaf_by_index, uint32_t* slot_by_index, void* nodes_out, size_t nodes_cap, size_t* n_nodes, int* max_depth) {
  if (!o) return CILHIP_ERR_INVALID;
  if (leaf_by_index && o->n) memcpy(leaf_by_index, o->leaf.data(), (size_t)o->n * sizeof(uint32_t));
  if (slot_by_index && o->n) memcpy(slot_by_index, o->slot.data(), (size_t)o->n * sizeof(uint32_t));
  if (nodes_out && nodes_cap) memcpy(nodes_out, o->nodes.data(), std::min(nodes_cap, o->nodes.size()) * sizeof(cilhip::TieNode));
  if (n_nodes) *n_nodes = o->nodes.size();
  if (max_depth) *max_depth = o->max_depth;
  return CILHIP_OK;
}
int cilhip_load_tie_order(cilhip_ctx* c, const cilhip_tie_order* order, const uint32_t* global_index) {
  if (!c || !order) return CILHIP_ERR_INVALID;
  if (!c->has_target) return fail(c, CILHIP_ERR_INVALID, "load_tie_order: set_target first");
  const uint32_t n = c->grid.n, N = order->n;
  if (n == 0) return load_tie_tables(c, nullptr, nullptr, order->nodes.data(), order->nodes.size());      // (a shard without target points)
  if (!global_index) {
    if (n != N) return fail(c, CILHIP_ERR_INVALID, "load_tie_order: the order was built for a cloud of another size (pass global_index for a part of it)");
    return load_tie_tables(c, order->leaf.data(), order->slot.data(), order->nodes.data(), order->nodes.size());
  }
  try {
    std::vector<uint32_t> leaf(n ? n : 1), slot(n ? n : 1);
    for (uint32_t i = 0; i < n; ++i) {
      if (global_index[i] >= N) return fail(c, CILHIP_ERR_INVALID, "load_tie_order: global index out of range");
      leaf[i] = order->leaf[global_index[i]]; slot[i] = order->slot[global_index[i]];
    }
    return load_tie_tables(c, leaf.data(), slot.data(), order->nodes.data(), order->nodes.size());
  } catch (...) { return fail(c, CILHIP_ERR_HIP, "load_tie_order: out of host memory"); }
}
int cilhip_build_tie_order(cilhip_ctx* c) {
  if (!c) return CILHIP_ERR_INVALID;
  if (!c->has_target) return fail(c, CILHIP_ERR_INVALID, "build_tie_order: set_target first");
  if (c->partial_target) return fail(c, CILHIP_ERR_INVALID, "build_tie_order: this context holds a PART of a target (cilhip_set_shard_info): the order is the whole cloud's -- cilhip_tie_order_create + cilhip_load_tie_order");
  return build_tie_tables(c);
}
int cilhip_get_tie_order_info(cilhip_ctx* c, cilhip_tie_order_info* out) {
  if (!c || !out) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  unsigned int cnt[4];
  { const int rc = read_tie_counters(c, cnt); if (rc) return rc; }
  out->loaded = (feat6(c) ? c->d_tief_leaf_slot != nullptr : c->d_tie_leaf_slot != nullptr) ? 1 : 0; out->builds = c->tie_builds + c->tief_builds; out->build_ms = c->tie_build_ms; out->pending = cnt[0];
  return CILHIP_OK;
}

int cilhip_get_tie_rule_stats(cilhip_ctx* c, size_t* tied_queries, size_t* repointed) {
  if (!c) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  unsigned int cnt[4];
  { const int rc = read_tie_counters(c, cnt); if (rc) return rc; }
  if (tied_queries) *tied_queries = (size_t)cnt[1] + (size_t)cnt[0] + (size_t)cnt[3];      // (settled from tables + met without them, forward and reverse)
  if (repointed) *repointed = (size_t)cnt[2];
  return CILHIP_OK;
}
