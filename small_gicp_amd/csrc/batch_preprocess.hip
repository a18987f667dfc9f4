// Batched preprocessing: sga_index_build_kdtree and sga_estimate_normals_covariances for B clouds of one context
// in one chain of launches.  A scan after the voxel grid (11 - 12k points) leaves the chip idle in every step of its lone build — level d
// of the tree is 2^d workgroups — and pays ~10 launches for ~100 us of kernels; B such scans fill the same launches B times over.
// The results are ordinary sga_index objects, each owning its buffers, bit-identical to what the lone calls produce: the batched
// kernels (index_build.hip, preprocess.hip) run the lone kernels' bodies with the arguments read from a per-call table (forest.hpp).
// sga_voxelgrid_sampling_batch does the same for the stage before them: B raw scans downsampled by one chain —
// keys, ONE sort over the concatenation under the key (member, the member's own short key), runs, centroids — and one host wait.
// sga_voxelmap_insert_batch: B scans into B incremental Gaussian maps by one chain and one host wait.
#include <atomic>
#include <memory>
#include <unordered_set>
#include <vector>

#include "common.hpp"
#include "forest.hpp"
#include "notes.hpp"
#include "voxel_steps.hpp"

namespace sga {
int build_cell_grid(sga_context* ctx, sga_index* idx);  // cell_grid.hip

static std::atomic<unsigned long long> g_launches[static_cast<int>(Chain::kCount)];
void count_launch(Chain chain) { g_launches[static_cast<int>(chain)].fetch_add(1, std::memory_order_relaxed); }
int report_launches(Chain chain, unsigned long long* launches) {
  if (!launches) return fail(SGA_ERR_INVALID, "null argument");
  *launches = g_launches[static_cast<int>(chain)].load(std::memory_order_relaxed);
  return SGA_OK;
}

// the context's box block grows to the call's need (grow-only; no call is in flight: every call waits for its boxes)
int forest_call_begin(sga_context* ctx, size_t members, size_t stride, unsigned long long* seq) {
  const size_t need = 4 + stride * members;
  *seq = ++ctx->forest_seq;
  if (ctx->forest_words >= need) return SGA_OK;
  if (ctx->h_forest) (void)hipHostFree(ctx->h_forest);
  ctx->h_forest = ctx->h_forest_dev = nullptr;
  ctx->forest_words = 0;
  size_t want = 1024;
  while (want < need) want <<= 1;
  if (hipHostMalloc(reinterpret_cast<void**>(&ctx->h_forest), want * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
    ctx->h_forest = nullptr;
    return fail(SGA_ERR_HIP, "hipHostMalloc(%zu bytes) failed", want * sizeof(unsigned long long));
  }
  std::memset(ctx->h_forest, 0, want * sizeof(unsigned long long));
  if (hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->h_forest_dev), ctx->h_forest, 0) != hipSuccess) return fail(SGA_ERR_HIP, "hipHostGetDevicePointer failed");
  ctx->forest_words = want;
  return SGA_OK;
}

// all slots are written once the block shows the call's sequence number (wait_published, context.hip)
int forest_call_wait(sga_context* ctx, int enqueued, unsigned long long seq, const char* what) {
  int rc = enqueued;
  if (rc == SGA_OK) {
    rc = wait_published(ctx, ctx->h_forest, seq);
    if (rc == kNotPublished) rc = fail(SGA_ERR_HIP, "the %s were not published by the device", what);
  }
  if (rc != SGA_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
  }
  return rc;
}

namespace {
int build_kdtrees(sga_context* ctx, const sga_cloud* const* clouds, size_t count, std::vector<std::unique_ptr<sga_index>>& made) {
  made.resize(count);
  std::vector<size_t> forest;  // positions of the members the forest builds: 1 <= n <= kForestMaxPoints
  size_t forest_points = 0;
  for (size_t k = 0; k < count; k++) {
    const sga_cloud* cloud = clouds[k];
    if (cloud->n == 0 || cloud->n > kForestMaxPoints) continue;  // the empty index below / the lone path
    SGA_TRY(wait_ready(ctx, cloud->ready));
    made[k] = kd_index_new(ctx, cloud);
    forest.push_back(k);
    forest_points += cloud->n;
  }
  DevBuf<uint32_t> perms;                 // the two permutation buffers of every tree
  DevBuf<unsigned long long> table;       // forest.hpp; both live until the end of the call (then: the stream's free list)
  unsigned long long seq = 0;
  if (!forest.empty()) {
    // ---- every allocation of every member, then the launches
    SGA_TRY(perms.alloc(2 * forest_points));
    SGA_TRY(forest_call_begin(ctx, forest.size(), kSlotWords, &seq));
    std::vector<ForestTree> trees(forest.size());
    size_t at = 0;
    for (size_t j = 0; j < forest.size(); j++) {
      const sga_cloud* cloud = clouds[forest[j]];
      sga_index* idx = made[forest[j]].get();
      const size_t n = cloud->n;
      int D = 0, dA = 0;
      forest_tree_shape(n, &D, &dA);
      idx->kd_depth = D;
      SGA_TRY(idx->kd_nodes.alloc(1ull << D));
      SGA_TRY(idx->kd_nodes4.alloc(kd_pair_count(D)));
      SGA_TRY(kd_index_alloc(idx, cloud, D));
      ForestTree& t = trees[j];
      std::memset(&t, 0, sizeof(t));
      t.pts = cloud->pts.p;
      t.nrm = cloud->has_normals ? cloud->nrm.p : nullptr;
      t.cov = cloud->has_covs ? cloud->cov.p : nullptr;
      t.perm[0] = perms.p + at;
      t.perm[1] = perms.p + at + n;
      at += 2 * n;
      t.nodes = idx->kd_nodes.p;
      t.opts = idx->kd_pts.p;
      t.onrm = idx->nrm.p;
      t.ocov = idx->cov.p;
      t.boxes = idx->kd_boxes.p;
      t.groups = idx->kd_groups.p;
      t.blocks = reinterpret_cast<float*>(idx->kd_leaf.p);
      t.pairs = idx->kd_nodes4.p;
      t.late_seq = late_note_begin(ctx->device, &t.late_slot);  // the length scale travels as a late note per index, as in the lone build
      idx->spacing = 0.0;
      idx->spacing_seq = t.late_seq;
      t.box_slot = forest_slot_dev(ctx, j);
      t.n = static_cast<uint32_t>(n);
      t.D = D;
      t.dA = dA;
    }
    // ---- the one wait: the boxes of all members
    SGA_TRY(forest_call_wait(ctx, forest_build(ctx, trees, ctx->h_forest_dev, seq, table), seq, "boxes of a batched kd-tree build"));
    for (size_t j = 0; j < forest.size(); j++) {
      sga_index* idx = made[forest[j]].get();
      box_note_decode(forest_slot_host(ctx, j) + kSlotBox, idx->bbox_lo, idx->bbox_hi);
      for (int a = 0; a < 3; a++)
        if (!std::isfinite(idx->bbox_lo[a]) || !std::isfinite(idx->bbox_hi[a])) return fail(SGA_ERR_INVALID, "target cloud %zu contains non-finite coordinates", forest[j]);
    }
    for (size_t k : forest) SGA_TRY(build_cell_grid(ctx, made[k].get()));  // (declines by its own rule for clouds this small)
  }
  // ---- the other members through the lone path, one after the other: empty clouds, clouds of more than kForestMaxPoints points
  for (size_t k = 0; k < count; k++) {
    if (made[k]) continue;
    sga_index* lone = nullptr;
    SGA_TRY(sga_index_build_kdtree(ctx, clouds[k], &lone));
    made[k].reset(lone);
  }
  if (!forest.empty() && !ctx->stream_ordered) SGA_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t k : forest) SGA_TRY(mark_ready(ctx, made[k]->ready));
  return SGA_OK;
}

// sga_voxelgrid_sampling for every member.  The members of the plan's forest share one chain of launches
// (preprocess.hip: grid_forest_enqueue) and ONE host wait, for their voxel counts; the others go through the lone routine afterwards.
int voxelgrid_batch(sga_context* ctx, const sga_cloud* const* clouds, size_t count, double leaf, std::vector<std::unique_ptr<sga_cloud>>& made) {
  made.resize(count);
  for (size_t k = 0; k < count; k++) {
    std::unique_ptr<sga_cloud> res(new sga_cloud);  // as sga_voxelgrid_sampling sets it up
    res->device = ctx->device;
    for (int a = 0; a < 3; a++) res->origin[a] = clouds[k]->origin[a];  // the centroids stay in the input's device frame
    SGA_TRY(wait_ready(ctx, clouds[k]->ready));
    made[k] = std::move(res);
  }
  const GridForestPlan plan = grid_forest_plan(clouds, count, leaf);
  if (!plan.forest.empty()) {
    std::vector<float4*> out(plan.forest.size());
    for (size_t j = 0; j < plan.forest.size(); j++) {
      sga_cloud* res = made[plan.forest[j]].get();
      SGA_TRY(res->pts.alloc(clouds[plan.forest[j]]->n));  // room for one voxel per point: the centroid kernel runs before the host knows the count
      out[j] = res->pts.p;
    }
    unsigned long long seq = 0;
    SGA_TRY(forest_call_begin(ctx, plan.forest.size(), kSlotWords, &seq));
    // ---- the one wait: the voxel counts of all forest members
    SGA_TRY(forest_call_wait(ctx, grid_forest_enqueue(ctx, clouds, leaf, plan, out.data(), seq), seq, "voxel counts of a batched voxel grid"));
    for (size_t j = 0; j < plan.forest.size(); j++) made[plan.forest[j]]->n = static_cast<size_t>(forest_slot_host(ctx, j)[kSlotRuns]);
  }
  // ---- the other members through the lone routine, one after the other: no box, more than 262144 points, past the forest's caps
  for (size_t k : plan.lone) {
    sga_cloud* lone = nullptr;
    SGA_TRY(sga_voxelgrid_sampling(ctx, clouds[k], leaf, &lone));
    made[k].reset(lone);
  }
  if (!plan.forest.empty() && !ctx->stream_ordered) SGA_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t k : plan.forest) SGA_TRY(mark_ready(ctx, made[k]->ready));
  return SGA_OK;
}

// the argument checks of sga_voxelgrid_sampling_batch and of its plan (status and message as the lone call's, naming the member)
int voxelgrid_batch_check(const sga_cloud* const* clouds, size_t count, double leaf) {
  if (!(leaf > 0)) return fail(SGA_ERR_INVALID, "leaf size must be positive");
  for (size_t k = 0; k < count; k++) {
    if (!clouds[k]) return fail(SGA_ERR_INVALID, "clouds[%zu] is NULL", k);
    if (clouds[k]->n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "cloud %zu too large (%zu points; limit 2^31-1)", k, clouds[k]->n);
  }
  return SGA_OK;
}
// the argument checks of sga_index_build_gaussian_voxelmap_batch and of its plan (status and message as the lone call's, naming the member)
int voxelmaps_batch_check(const sga_cloud* const* clouds, size_t count, double leaf) {
  if (!(leaf > 0)) return fail(SGA_ERR_INVALID, "leaf size must be positive");
  for (size_t k = 0; k < count; k++) {
    if (!clouds[k]) return fail(SGA_ERR_INVALID, "clouds[%zu] is NULL", k);
    if (!clouds[k]->has_covs) return fail(SGA_ERR_INVALID, "GaussianVoxelMap needs point covariances (cloud %zu)", k);
  }
  return SGA_OK;
}

// sga_index_build_gaussian_voxelmap for every member.  The members of the plan's chain share the launches
// (voxelmap_build.hip: vox_forest_enqueue_runs, vox_forest_enqueue_finalize) and ONE host wait, for their voxel counts and overflow words;
// behind it every index is allocated at its exact size.  Members the plan leaves out, and members whose key overflowed, go through the
// lone routine afterwards.
int voxelmaps_batch(sga_context* ctx, const sga_cloud* const* clouds, size_t count, double leaf, std::vector<std::unique_ptr<sga_index>>& made) {
  made.resize(count);
  for (size_t k = 0; k < count; k++) SGA_TRY(wait_ready(ctx, clouds[k]->ready));
  const VoxForestPlan plan = vox_forest_plan(clouds, count);
  VoxelForestChain ch;
  std::vector<size_t> lone = plan.lone;
  std::vector<VoxMember> members;  // of the stage behind the wait
  std::vector<size_t> built;       // their positions in the call
  auto add_member = [&](size_t k, uint32_t nvox, uint32_t off, uint32_t run0) -> int {
    const sga_cloud* cloud = clouds[k];
    std::unique_ptr<sga_index> idx;
    SGA_TRY(gaussian_map_new(ctx, cloud, leaf, nvox, idx));
    SGA_TRY(gaussian_map_alloc_voxels(idx.get()));
    VoxMember g;
    std::memset(&g, 0, sizeof(g));
    g.pts = cloud->pts.p;
    g.cov = cloud->cov.p;
    g.ox = cloud->origin[0], g.oy = cloud->origin[1], g.oz = cloud->origin[2];
    g.n = static_cast<uint32_t>(cloud->n);
    g.off = off;
    g.means = idx->pts.p;
    g.mcov = idx->cov.p;
    g.coords = idx->vcoords.p;
    g.counts = idx->vcounts.p;
    g.hkeys = idx->hkeys.p;
    g.hvals = idx->hvals.p;
    g.hmask = idx->hmask;
    g.nvox = nvox;
    g.run0 = run0;
    members.push_back(g);
    built.push_back(k);
    made[k] = std::move(idx);
    return SGA_OK;
  };
  size_t runs = 0;
  if (!plan.forest.empty()) {
    unsigned long long seq = 0;
    SGA_TRY(forest_call_begin(ctx, plan.forest.size(), kSlotWords, &seq));
    // ---- the one wait: the voxel counts and overflow words of all members of the chain
    SGA_TRY(forest_call_wait(ctx, vox_forest_enqueue_runs(ctx, clouds, leaf, plan, seq, ch), seq, "voxel counts of a batched voxel-map build"));
    uint32_t off = 0;
    for (size_t j = 0; j < plan.forest.size(); j++) {
      const size_t k = plan.forest[j];
      const unsigned long long nvox = forest_slot_host(ctx, j)[kSlotRuns], overflow = forest_slot_host(ctx, j)[kSlotOverflow];
      if (nvox > clouds[k]->n) return fail(SGA_ERR_HIP, "the device reported %llu voxels for the %zu points of cloud %zu", nvox, clouds[k]->n, k);
      if (overflow)
        lone.push_back(k);  // two voxels of the member may have shared a key: what the chain made of it is dropped
      else
        SGA_TRY(add_member(k, static_cast<uint32_t>(nvox), off, static_cast<uint32_t>(runs)));
      off += static_cast<uint32_t>(clouds[k]->n);
      runs += nvox;  // (the runs are numbered over the whole chain, an overflowed member's included)
    }
  }
  for (size_t k : plan.empty) SGA_TRY(add_member(k, 0u, 0u, 0u));  // an empty map: its 16-slot table is cleared with the others
  SGA_TRY(vox_forest_enqueue_finalize(ctx, members, runs, leaf, ch));
  // ---- the other members through the lone routine, one after the other
  for (size_t k : lone) {
    sga_index* one = nullptr;
    SGA_TRY(sga_index_build_gaussian_voxelmap(ctx, clouds[k], leaf, &one));
    made[k].reset(one);
  }
  if (!built.empty() && !ctx->stream_ordered) SGA_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t k : built) SGA_TRY(mark_ready(ctx, made[k]->ready));
  return SGA_OK;
}
// the argument checks of sga_voxelmap_insert_batch and of its plan that need no context (status and message as the lone call's, naming the member)
int insert_batch_check(sga_index* const* maps, const sga_cloud* const* clouds, size_t count) {
  std::unordered_set<const void*> seen;
  for (size_t k = 0; k < count; k++) {
    if (!maps[k]) return fail(SGA_ERR_INVALID, "null argument: maps[%zu] is NULL", k);
    if (!clouds[k]) return fail(SGA_ERR_INVALID, "null argument: clouds[%zu] is NULL", k);
    const sga_index* idx = maps[k];
    const sga_cloud* cloud = clouds[k];
    if (!idx->incremental) return fail(SGA_ERR_INVALID, "not an incremental voxel map (create it with sga_voxelmap_create) (member %zu)", k);
    if ((idx->kind != SGA_INDEX_FLATMAP || idx->has_covs) && cloud->n > 0 && !cloud->has_covs) return fail(SGA_ERR_INVALID, "GaussianVoxelMap needs point covariances (member %zu)", k);
    if (idx->kind == SGA_INDEX_FLATMAP && idx->has_normals && cloud->n > 0 && !cloud->has_normals) return fail(SGA_ERR_INVALID, "a flat voxel map with normals needs point normals (member %zu)", k);
    if (!seen.insert(idx).second) return fail(SGA_ERR_INVALID, "map %zu appears twice in the batch (two inserts into one map are ordered: make two calls)", k);
  }
  return SGA_OK;
}

// sga_voxelmap_insert for every member.  The members of the plan's chain share the launches (voxelmap.hip:
// ivm_forest_enqueue_runs / _update / _export) and ONE host wait, for their run counts, new-voxel counts and overflow words; behind it
// every map grows under the lone call's conditions.  Sweeps run one map at a time; the fp32 records of all maps are exported by one
// launch.  Flat maps, larger clouds and members whose key overflowed go through the lone routine afterwards.
int insert_batch(sga_context* ctx, sga_index* const* maps, const sga_cloud* const* clouds, const double* T, size_t count) {
  for (size_t k = 0; k < count; k++) {
    SGA_TRY(wait_ready(ctx, clouds[k]->ready));
    SGA_TRY(wait_ready(ctx, maps[k]->ready));
  }
  const IvmForestPlan plan = ivm_forest_plan(maps, clouds, count);
  VoxelForestChain ch;
  std::vector<size_t> lone = plan.lone;
  std::vector<size_t> own;  // the maps whose counter, sweep and export are this call's: the chain's members that did not overflow, and the empty ones
  if (!plan.forest.empty()) {
    const size_t B = plan.forest.size();
    unsigned long long seq = 0;
    SGA_TRY(forest_call_begin(ctx, B, kSlotWords, &seq));
    // ---- the one wait: run counts, overflow words and new-voxel counts of all members of the chain
    SGA_TRY(forest_call_wait(ctx, ivm_forest_enqueue_runs(ctx, maps, clouds, T, plan, seq, ch), seq, "voxel counts of a batched voxel-map insert"));
    std::vector<uint32_t> nseg(B), n_new(B);
    std::vector<bool> overflow(B);
    size_t runs = 0, total_new = 0;
    for (size_t j = 0; j < B; j++) {
      const size_t k = plan.forest[j];
      const unsigned long long* slot = forest_slot_host(ctx, j);
      const unsigned long long s = slot[kSlotRuns], w = slot[kSlotNewVoxels];
      if (s > clouds[k]->n || w > s) return fail(SGA_ERR_HIP, "the device reported %llu voxels (%llu new) for the %zu points of cloud %zu", s, w, clouds[k]->n, k);
      nseg[j] = static_cast<uint32_t>(s);
      n_new[j] = static_cast<uint32_t>(w);
      overflow[j] = slot[kSlotOverflow] != 0;
      runs += s;
      total_new += w;
      if (!overflow[j] && maps[k]->n + w >= (1ull << 31)) return fail(SGA_ERR_INVALID, "voxel map too large (member %zu)", k);
    }
    // ---- capacity, then the second table: the pointers after growth, each member's place in the ranks' order
    std::vector<IvmUpdate> members;
    uint32_t off = 0, new0 = 0, old0 = 0;
    for (size_t j = 0; j < B; j++) {
      const size_t k = plan.forest[j];
      sga_index* idx = maps[k];
      const sga_cloud* cloud = clouds[k];
      if (overflow[j]) {
        lone.push_back(k);  // two voxels of the member may have shared a key: the chain writes nothing of it
      } else {
        own.push_back(k);
        if (nseg[j] > 0) {
          SGA_TRY(ivm_reserve(ctx, idx, idx->n + n_new[j]));
          IvmUpdate g;
          std::memset(&g, 0, sizeof(g));
          g.pts = cloud->pts.p;
          g.cov = cloud->cov.p;
          g.T = insert_pose(T ? T + 16 * k : nullptr, cloud->origin);
          g.inv_leaf = 1.0 / idx->leaf;
          g.mean64 = idx->vmean64.p;
          g.cov64 = idx->vcov64.p;
          g.counts = idx->vcounts.p;
          g.lru = idx->vlru.p;
          g.coords = idx->vcoords.p;
          g.hkeys = idx->hkeys.p;
          g.hvals = idx->hvals.p;
          g.hmask = idx->hmask;
          g.n_old = static_cast<uint32_t>(idx->n);
          g.lru_counter = idx->lru_counter;
          g.nseg = nseg[j];
          g.n_new = n_new[j];
          g.new0 = new0;
          g.old0 = old0;
          g.end = off + static_cast<uint32_t>(cloud->n);
          members.push_back(g);
        }
      }
      off += static_cast<uint32_t>(cloud->n);
      new0 += n_new[j];  // (the runs of an overflowed member stay in the ranks' order)
      old0 += nseg[j] - n_new[j];
    }
    SGA_TRY(ivm_forest_enqueue_update(ctx, members, runs, static_cast<uint32_t>(total_new), B, ch));
    for (size_t j = 0; j < B; j++)
      if (!overflow[j]) maps[plan.forest[j]]->n += n_new[j];
  }
  own.insert(own.end(), plan.empty.begin(), plan.empty.end());
  // ---- LRU sweeps (rare: one map at a time), then the fp32 records of every map by one launch
  for (size_t k : own) {
    maps[k]->lru_counter++;
    SGA_TRY(ivm_lru_sweep(ctx, maps[k]));
  }
  std::vector<IvmExport> exports;
  std::vector<double> origins(3 * own.size());
  for (size_t i = 0; i < own.size(); i++) {
    const sga_index* idx = maps[own[i]];
    const sga_cloud* cloud = clouds[own[i]];
    double* o = origins.data() + 3 * i;
    map_origin_after_insert(insert_pose(T ? T + 16 * own[i] : nullptr, cloud->origin), cloud->n, 1.0 / idx->leaf, idx->origin, o);  // as in the lone call
    if (idx->n == 0) continue;
    IvmExport e;
    std::memset(&e, 0, sizeof(e));
    e.mean64 = idx->vmean64.p;
    e.cov64 = idx->vcov64.p;
    e.means = idx->pts.p;
    e.mcov = idx->cov.p;
    e.ox = o[0], e.oy = o[1], e.oz = o[2];
    e.n = static_cast<uint32_t>(idx->n);
    exports.push_back(e);
  }
  SGA_TRY(ivm_forest_enqueue_export(ctx, exports, ch));
  for (size_t i = 0; i < own.size(); i++)  // every fallible step of these maps is behind us: the records enqueued are relative to the new origin
    for (int a = 0; a < 3; a++) maps[own[i]]->origin[a] = origins[3 * i + a];
  // ---- the other members through the lone routine, one after the other
  for (size_t k : lone) SGA_TRY(sga_voxelmap_insert(ctx, maps[k], clouds[k], T ? T + 16 * k : nullptr));
  if (!own.empty() && !ctx->stream_ordered) SGA_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t k : own) SGA_TRY(mark_ready(ctx, maps[k]->ready));
  return SGA_OK;
}
}  // namespace

}  // namespace sga

using namespace sga;

extern "C" {

int sga_debug_forest_launches(unsigned long long* launches) { return report_launches(Chain::Forest, launches); }

int sga_debug_voxelgrid_batch_launches(unsigned long long* launches) { return report_launches(Chain::Grid, launches); }

int sga_debug_voxelgrid_batch_plan(const sga_cloud* const* clouds, size_t count, double leaf, int out[6]) {
  if (!out || (count > 0 && !clouds)) return fail(SGA_ERR_INVALID, "null argument");
  for (int k = 0; k < 6; k++) out[k] = 0;
  SGA_TRY(voxelgrid_batch_check(clouds, count, leaf));
  const GridForestPlan P = grid_forest_plan(clouds, count, leaf);
  out[0] = P.key_bytes;
  out[1] = P.W;
  out[2] = P.member_bits;
  out[3] = static_cast<int>(P.forest.size());
  out[4] = static_cast<int>(P.lone.size());
  out[5] = static_cast<int>(P.tiles);
  return SGA_OK;
}

int sga_voxelgrid_sampling_batch(sga_context* ctx, const sga_cloud* const* clouds, size_t count, double leaf, sga_cloud** out) {
  if (count == 0) return SGA_OK;
  null_out(out, count);
  if (!ctx || !clouds || !out) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(voxelgrid_batch_check(clouds, count, leaf));
  for (size_t k = 0; k < count; k++)
    if (clouds[k]->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud %zu lives on another device", k);
  SGA_ENTER(ctx);
  return build_into(out, [&](std::vector<std::unique_ptr<sga_cloud>>& made) { return voxelgrid_batch(ctx, clouds, count, leaf, made); });
}

int sga_debug_voxelmap_batch_launches(unsigned long long* launches) { return report_launches(Chain::VoxBuild, launches); }

static int report_plan(const VoxForestPlan& P, int out[6]) {
  out[0] = static_cast<int>(P.forest.size());
  out[1] = static_cast<int>(P.lone.size());
  out[2] = static_cast<int>(P.empty.size());
  out[3] = P.member_bits;
  out[4] = P.end_bit;
  out[5] = static_cast<int>(P.points);
  return SGA_OK;
}

int sga_debug_voxelmap_batch_plan(const sga_cloud* const* clouds, size_t count, double leaf, int out[6]) {
  if (!out || (count > 0 && !clouds)) return fail(SGA_ERR_INVALID, "null argument");
  for (int k = 0; k < 6; k++) out[k] = 0;
  SGA_TRY(voxelmaps_batch_check(clouds, count, leaf));
  return report_plan(vox_forest_plan(clouds, count), out);
}

int sga_index_build_gaussian_voxelmap_batch(sga_context* ctx, const sga_cloud* const* clouds, size_t count, double leaf, sga_index** out) {
  if (count == 0) return SGA_OK;
  null_out(out, count);
  if (!ctx || !clouds || !out) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(voxelmaps_batch_check(clouds, count, leaf));
  for (size_t k = 0; k < count; k++)
    if (clouds[k]->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud %zu lives on another device", k);
  SGA_ENTER(ctx);
  return build_into(out, [&](std::vector<std::unique_ptr<sga_index>>& made) { return voxelmaps_batch(ctx, clouds, count, leaf, made); });
}

int sga_debug_voxelmap_insert_batch_launches(unsigned long long* launches) { return report_launches(Chain::IvmInsert, launches); }

int sga_debug_voxelmap_insert_batch_plan(sga_index* const* maps, const sga_cloud* const* clouds, size_t count, int out[6]) {
  if (!out || (count > 0 && (!maps || !clouds))) return fail(SGA_ERR_INVALID, "null argument");
  for (int k = 0; k < 6; k++) out[k] = 0;
  SGA_TRY(insert_batch_check(maps, clouds, count));
  return report_plan(ivm_forest_plan(maps, clouds, count), out);
}

int sga_voxelmap_insert_batch(sga_context* ctx, sga_index* const* maps, const sga_cloud* const* clouds, const double* T, size_t count) {
  if (count == 0) return SGA_OK;
  if (!ctx || !maps || !clouds) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(insert_batch_check(maps, clouds, count));
  for (size_t k = 0; k < count; k++)
    if (clouds[k]->device != ctx->device || maps[k]->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud / map live on another device (member %zu)", k);
  SGA_ENTER(ctx);
  return insert_batch(ctx, maps, clouds, T, count);
}

int sga_index_build_kdtree_batch(sga_context* ctx, const sga_cloud* const* clouds, size_t count, sga_index** out) {
  if (count == 0) return SGA_OK;
  null_out(out, count);
  if (!ctx || !clouds || !out) return fail(SGA_ERR_INVALID, "null argument");
  for (size_t k = 0; k < count; k++) {
    if (!clouds[k]) return fail(SGA_ERR_INVALID, "clouds[%zu] is NULL", k);
    if (clouds[k]->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud %zu lives on another device", k);
  }
  SGA_ENTER(ctx);
  return build_into(out, [&](std::vector<std::unique_ptr<sga_index>>& made) { return build_kdtrees(ctx, clouds, count, made); });
}

int sga_estimate_normals_covariances_batch(sga_context* ctx, sga_cloud* const* clouds, sga_index* const* indices, size_t count, int k, int flags) {
  if (count == 0) return SGA_OK;
  SGA_TRY(features_check_k(k));
  if (!ctx || !clouds || !indices) return fail(SGA_ERR_INVALID, "null argument");
  std::unordered_set<const void*> seen;
  for (size_t m = 0; m < count; m++) {
    const sga_cloud* cloud = clouds[m];
    const sga_index* index = indices[m];
    if (!cloud) return fail(SGA_ERR_INVALID, "clouds[%zu] is NULL", m);
    if (!index) return fail(SGA_ERR_INVALID, "indices[%zu] is NULL (a batched estimation needs the index of every cloud)", m);
    if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud %zu lives on another device", m);
    if (index->device != ctx->device) return fail(SGA_ERR_INVALID, "index %zu lives on another device", m);
    if (index->kind == SGA_INDEX_PROJECTIVE) return fail(SGA_ERR_UNSUPPORTED, "normal / covariance estimation needs a kd-tree index, not a projective search (member %zu)", m);
    if (index->kind != SGA_INDEX_KDTREE) return fail(SGA_ERR_INVALID, "a kd-tree index is required (member %zu)", m);
    if (index->n != cloud->n) return fail(SGA_ERR_INVALID, "index %zu was built over a cloud of %zu points, got %zu", m, index->n, cloud->n);
    for (int a = 0; a < 3; a++)
      if (index->origin[a] != cloud->origin[a]) return fail(SGA_ERR_INVALID, "index %zu was not built over its cloud (their device frames differ)", m);
    if (!seen.insert(cloud).second) return fail(SGA_ERR_INVALID, "cloud %zu appears twice in the batch", m);
    if (!seen.insert(index).second) return fail(SGA_ERR_INVALID, "index %zu appears twice in the batch", m);
  }
  if ((flags & 3) == 0) return SGA_OK;
  SGA_ENTER(ctx);
  // the forest form is knn_wave_kernel + features_from_list_kernel: the members the lone routine gives those two kernels
  const long long wave_max = knn_wave_max_points();
  std::vector<size_t> forest;
  unsigned long long blocks = 0;
  for (size_t m = 0; m < count; m++) {
    const size_t n = clouds[m]->n;
    if (n == 0 || static_cast<long long>(n) > wave_max || k > 64 || blocks + n > 0x7fffffffull) continue;
    forest.push_back(m);
    blocks += n;
  }
  DevBuf<int> nbr;
  DevBuf<unsigned long long> table;
  if (!forest.empty()) {
    std::vector<ForestFeat> members(forest.size());
    SGA_TRY(nbr.alloc(blocks * static_cast<size_t>(k)));
    size_t at = 0;
    for (size_t j = 0; j < forest.size(); j++) {
      sga_cloud* cloud = clouds[forest[j]];
      sga_index* index = indices[forest[j]];
      const size_t n = cloud->n;
      SGA_TRY(wait_ready(ctx, index->ready));
      SGA_TRY(wait_ready(ctx, cloud->ready));
      if ((flags & 1) && cloud->nrm.n < n) SGA_TRY(cloud->nrm.alloc(n));
      if ((flags & 2) && cloud->cov.n < n) SGA_TRY(cloud->cov.alloc(n));
      if ((flags & 1) && index->nrm.n < n) SGA_TRY(index->nrm.alloc(n));
      if ((flags & 2) && index->cov.n < n) SGA_TRY(index->cov.alloc(n));
      ForestFeat& f = members[j];
      f.g = make_kd_view(index);
      f.nbr = nbr.p + at;
      at += n * static_cast<size_t>(k);
      f.idx_nrm = index->nrm.p;
      f.idx_cov = index->cov.p;
      f.cloud_nrm = cloud->nrm.p;
      f.cloud_cov = cloud->cov.p;
      f.ox = cloud->origin[0], f.oy = cloud->origin[1], f.oz = cloud->origin[2];
    }
    SGA_TRY(forest_features(ctx, members, k, flags, table));
  }
  // the other members through the lone routine: empty clouds, clouds above the one-wave-per-query limit, k > 64
  for (size_t m = 0, j = 0; m < count; m++) {
    if (j < forest.size() && forest[j] == m) {
      j++;
      continue;
    }
    SGA_TRY(sga_estimate_normals_covariances(ctx, clouds[m], indices[m], k, flags));
  }
  if (!forest.empty() && !ctx->stream_ordered) SGA_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t m : forest) {
    if (flags & 1) clouds[m]->has_normals = indices[m]->has_normals = true;
    if (flags & 2) clouds[m]->has_covs = indices[m]->has_covs = true;
    SGA_TRY(mark_ready(ctx, indices[m]->ready));
    SGA_TRY(mark_ready(ctx, clouds[m]->ready));
  }
  return SGA_OK;
}

}  // extern "C"
