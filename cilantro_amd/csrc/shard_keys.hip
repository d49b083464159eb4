// shard_keys.hip -- what a context is told about the part of a sharded run it holds (cilhip_set_shard_info, the slab guard) and the key
// exchange between target shards (cilhip_icp_partial_keys / _sums_from_keys / _order_keys / _sums_from_ordered_keys).
#include <cstddef>
#include <cstring>

#include "ctx.hpp"

int cilhip_set_shard_info(cilhip_ctx* c, uint64_t target_index_offset, const float* dst_mean, const float* src_mean) {
  if (!c) return CILHIP_ERR_INVALID;
  if (target_index_offset + (c->has_target ? c->grid.n : 0) > 0xFFFFFFFFull) return fail(c, CILHIP_ERR_INVALID, "global target indices must fit 32 bits");
  c->index_offset = (uint32_t)target_index_offset;
  c->partial_target = target_index_offset != 0 || dst_mean != nullptr;      // (the whole cloud's mean handed in: this target is a part of it)
  if (dst_mean) memcpy(c->dst_mean, dst_mean, sizeof(c->dst_mean));
  if (src_mean) memcpy(c->src_mean, src_mean, sizeof(c->src_mean));
  return CILHIP_OK;
}

int cilhip_set_slab_guard(cilhip_ctx* c, int axis, float slack, const float center[3], const float half_extent[3], const float T_part[16]) {
  if (!c) return CILHIP_ERR_INVALID;
  if (axis < 0) { c->guard_axis = -1; return CILHIP_OK; }
  if (axis > 2 || !center || !half_extent || !T_part || !(slack >= 0.0f)) return fail(c, CILHIP_ERR_INVALID, "set_slab_guard: axis 0..2, slack >= 0, box and transform required");
  c->guard_axis = axis; c->guard_slack = slack;
  memcpy(c->guard_center, center, sizeof(c->guard_center)); memcpy(c->guard_half, half_extent, sizeof(c->guard_half));
  memcpy(c->guard_T, T_part, sizeof(c->guard_T));
  return CILHIP_OK;
}

int cilhip_get_slab_violation(cilhip_ctx* c, int* out) {
  if (!c || !out) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  int v = 0;
  CK(c, hipMemcpyAsync(&v, reinterpret_cast<const char*>(c->d_state.get()) + offsetof(IcpState, slab_violation), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  *out = v;
  return CILHIP_OK;
}

int cilhip_get_slab_violation_state(cilhip_ctx* c, int* violated, cilhip_icp_result* at) {
  if (!c || !violated) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  IcpState hs;
  CK(c, hipMemcpyAsync(&hs, c->d_state, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  *violated = hs.slab_violation;
  if (at) {
    memcpy(at->T, hs.slab_violation ? hs.violation_T : hs.T, sizeof(hs.T));
    at->iterations = (size_t)(hs.slab_violation ? hs.violation_iter : hs.iterations);
    at->last_delta_norm = hs.slab_violation ? hs.violation_delta : hs.delta;
    at->last_ncorr = (size_t)(hs.slab_violation ? hs.violation_ncorr : hs.ncorr);
  }
  return CILHIP_OK;
}

int cilhip_icp_partial_keys(cilhip_ctx* c, uint64_t* keys_dev) {
  if (!c || !keys_dev) return CILHIP_ERR_INVALID;
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  CK(c, hipSetDevice(c->device));
  IterArgs a = make_iter_args(c, c->run_prm.max_sq_dist);
  if (c->ns) {
    if (c->grid.n == 0) CK(c, hipMemsetAsync(c->d_nn_pos, 0xFF, (size_t)c->ns * sizeof(uint32_t), c->stream));      // (a shard without target points: every key "none")
    else if (use_tiled(c)) launch_search_tiled(a, IM_NONE, c->d_tiles, c->d_tile_center, c->d_tile_box, c->ntiles, c->stream);
    else launch_iter(a, IM_NONE, true, true, iter_num_blocks(c->ns), c->stream);
    launch_pack_keys(c->d_src_sorted, c->grid.pts, c->d_nn_pos, c->d_nn_d2, c->ns, c->index_offset,
                     reinterpret_cast<unsigned long long*>(keys_dev), c->stream);
  }
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

// the sums over the matches a key exchange has just selected into nn_pos / nn_d2 (select: enqueues that selection)
template <class Select>
static int sums_of_selected(cilhip_ctx* c, double* sums_dev, Select select) {
  const int im = iter_metric_of(c, &c->run_prm);
  IterArgs a = make_iter_args(c, c->run_prm.max_sq_dist);
  a.cw = corr_weights_of(c, &c->run_prm);
  const int nb = iter_num_blocks(c->ns);
  if (c->ns && c->grid.n) {
    select();
    launch_iter(a, im, false, false, nb, c->stream);
    launch_reduce_partials(c->d_partials, nb, c->d_stage, sums_dev, c->stream);
  } else {
    CK(c, hipMemsetAsync(sums_dev, 0, SUMS_MAX * sizeof(double), c->stream));
  }
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

int cilhip_icp_sums_from_keys(cilhip_ctx* c, const uint64_t* keys_dev, double* sums_dev) {
  if (!c || !keys_dev || !sums_dev) return CILHIP_ERR_INVALID;
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  CK(c, hipSetDevice(c->device));
  if (!c->d_inv_perm) {
    CK(c, c->d_inv_perm.alloc(c->grid.n));
    launch_inv_perm(c->grid.pts, c->grid.n, c->d_inv_perm, c->stream);
  }
  return sums_of_selected(c, sums_dev, [&] {
    launch_keys_to_pos(c->d_src_sorted, reinterpret_cast<const unsigned long long*>(keys_dev), c->d_inv_perm, c->ns,
                       c->index_offset, c->grid.n, c->d_nn_pos, c->d_nn_d2, c->stream,
                       (tie_mode_on(c) && !c->d_tie_leaf_slot) ? c->d_tie_counters : nullptr); });
}

// The reference's tie order across target shards (extract.hip: tie_rank): after the MIN all-reduce of cilhip_icp_partial_keys' keys,
//   cilhip_icp_order_keys(ctx, win_keys_dev, order_keys_dev)   order_keys_dev[i] = where this shard's match of source point i comes in
//                                                              the query's traversal of the WHOLE target's tree, if it is at the
//                                                              winning distance; 0x7fff...f otherwise
//   all-reduce(MIN, 64-bit) of order_keys_dev                  -> the first-met point of the whole target
//   cilhip_icp_sums_from_ordered_keys(ctx, win_keys_dev, order_keys_dev, sums_dev)   accumulates the pairs whose key came back
// Needs the whole target's order tables on every shard (cilhip_load_tie_order with the shard's global indices).
int cilhip_icp_order_keys(cilhip_ctx* c, const uint64_t* win_keys_dev, uint64_t* order_keys_dev) {
  if (!c || !win_keys_dev || !order_keys_dev) return CILHIP_ERR_INVALID;
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  if (!c->d_tie_leaf_slot) return fail(c, CILHIP_ERR_INVALID, "icp_order_keys: load the whole target's tie order first (cilhip_load_tie_order)");
  if (c->tie_max_depth > 58) return fail(c, CILHIP_ERR_UNSUPPORTED, "icp_order_keys: the order tree is deeper than the 58 levels a traversal key holds");
  CK(c, hipSetDevice(c->device));
  if (!c->d_own_order) CK(c, c->d_own_order.alloc(c->ns));
  TieDev t = tie_dev_of(c);
  launch_order_keys(c->d_src_sorted, c->d_state, reinterpret_cast<const unsigned long long*>(win_keys_dev), c->d_nn_pos, c->d_nn_d2, c->ns, t,
                    c->d_own_order, reinterpret_cast<unsigned long long*>(order_keys_dev), c->stream);
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

int cilhip_icp_sums_from_ordered_keys(cilhip_ctx* c, const uint64_t* win_keys_dev, const uint64_t* order_keys_dev, double* sums_dev) {
  if (!c || !win_keys_dev || !order_keys_dev || !sums_dev) return CILHIP_ERR_INVALID;
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  if (!c->d_own_order) return fail(c, CILHIP_ERR_INVALID, "icp_sums_from_ordered_keys: cilhip_icp_order_keys first");
  CK(c, hipSetDevice(c->device));
  return sums_of_selected(c, sums_dev, [&] {
    launch_select_ordered(c->d_src_sorted, c->d_own_order, reinterpret_cast<const unsigned long long*>(order_keys_dev),
                          reinterpret_cast<const unsigned long long*>(win_keys_dev), c->ns, c->d_nn_pos, c->d_nn_d2, c->stream); });
}
