// ssf_internal.hpp -- host-side context and kernel-launch declarations (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/ssf_frontend.h"

namespace ssf {

// Device scratch owned by a context: grown on demand, never shrunk, released with its owner.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            if (e != hipSuccess) return e;
            p = nullptr; bytes = 0;
        }
        size_t want = need + need / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = want;
        return hipSuccess;
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// Kernel timing (ssf_profile_enable): a launcher calls kmark(stream, "k_name") right before
// each kernel it launches; the ABI entry that owns those launches closes the last interval.
// With timing off (the default) kmark is one thread-local load and a branch.
void kmark(hipStream_t s, const char* name);

#ifndef SSF_BIN_CHUNK
#define SSF_BIN_CHUNK 2048
#endif
constexpr int kBinChunk = SSF_BIN_CHUNK;   // points per binning work-group (2048: 8 points per
                                           // thread; 4096 measured 11-12 % slower binning)
constexpr int kMaxRows = 64;
#ifndef SSF_MASK_MAX_SPLIT
#define SSF_MASK_MAX_SPLIT 32
#endif
constexpr int kMaskMaxSplit = SSF_MASK_MAX_SPLIT;   // work-groups per frame of the GMM fit at most
// scratch of the binned feature stage (feat_bin.hip): the candidate flag bytes of a batch
// (k_bin_curv -> k_select, one per ring position, per frame 64-byte aligned) and the curvature
// fix-up lists (per-frame counts, then ring positions at the frame offsets)
size_t flag_bytes(int64_t total, int n_frames);
size_t fix_bytes(int64_t total, int n_frames);

// Per-correspondence record written by the association kernel, read by the solver.
struct alignas(16) CorrRec {
    float po[3]; float valid;   // current-frame point (untransformed), 1 if the plane is valid
    float pa[3]; float pad0;    // last-frame 1-NN point
    float n[3];  float pad1;    // plane normal (float, as matX0)
};

// ---- the feature stage: its arguments, scratch sizes and launcher (features.hip) ----
// Edge selection of launch_extract_planes (beyond the reference; nullptr = planes only):
// the per-row selection slots in ctx scratch, the compacted edge cloud (float4 x, y, z,
// intensity at the frame offsets) and per-frame counts out (the candidates ride in bit 1 of
// the planar flag bytes).
struct EdgeSel {
    float min_curv;
    int span;
    int32_t* sel;
    float4* out;
    int32_t* count;
};
// Scratch of the single-read feature stage (feat_wave.hip, feat_chunk.hip, feat_select.hip;
// frames of at most 128 chunks): per-(chunk, row) counts -> row bases, u16 chunk positions per
// own-tile slot, the chunks' candidate / unresolved / edge bit planes, (debug outputs only)
// chunk-major curvature, and which kernel did each (frame, chunk) block.
struct FeatScratch {
    const void* rtab;   // the ring-id table (build_ring_table), device copy
    int32_t* cnt;       // feat_cnt_bytes
    uint16_t* gidx;     // feat_idx_bytes
    uint64_t* gbits;    // feat_bits_bytes
    float* curv_cm;     // total floats (debug), else nullptr
    uint8_t* irr;       // feat_irr_bytes: per (frame, chunk) block, the kernel that did it (kIrr*)
    uint8_t* lmap;      // feat_lmap_bytes: per regular block, row -> lane (64 B)
};
size_t feat_idx_bytes(int64_t total, int n_frames);
size_t feat_bits_bytes(int n_frames, int64_t max_pts);
size_t feat_cnt_bytes(int n_frames, int64_t max_pts);
size_t feat_irr_bytes(int n_frames, int64_t max_pts);
size_t feat_lmap_bytes(int n_frames, int64_t max_pts);
bool feat_single_read(int64_t max_pts);
// Scratch that only the binned stage reads (feat_bin.hip: k_bin_count / k_bin_scan / k_bin_curv /
// k_select, frames beyond the single-read capacity).
struct BinScratch {
    int8_t* rid;        // ring id per input point (total bytes)
    int32_t* hist;      // per (frame, chunk, row) counts
    int32_t* ring_idx;  // input index per ring position (total)
    uint8_t* flags;     // flag_bytes
    void* fix;          // fix_bytes
};
// The input frames of launch_extract_planes (pts: stride floats per point, xyz first; keep: the
// per-point mask, nullable) ...
struct FeatFrames {
    const float* pts;
    int stride;
    const int64_t* frame_off;
    int64_t max_pts;
    const uint8_t* keep;
};
// ... and its outputs: the plane clouds and per-frame counts, the ring offsets, and the debug
// outputs (ring-ordered points and curvature, nullable).
struct FeatOut {
    float4* plane;
    int32_t* plane_count;
    int32_t* ring_off;
    float4* ring_xyzi;
    float* curv;
};
// sel: the per-row selection slots (total int32, ctx scratch); edge: nullptr = planes only.
hipError_t launch_extract_planes(hipStream_t s, const ssf_config& cfg, int n_frames,
                                 const FeatFrames& in, const FeatOut& out, int32_t* sel,
                                 const BinScratch& bin, const FeatScratch& fs, const EdgeSel* edge);
// launch_extract_planes' stages, each beside its kernels; launch_extract_planes checks for
// errors.  What they share: the launch's arguments, n_chunks (the chunks of the largest frame),
// dbg (the debug outputs are asked for: the <kDebug> instantiations) and the edge selection --
// es holds the values the kernels are passed when it is off (edge = false).
struct FeatLaunch {
    hipStream_t s;
    const ssf_config& cfg;
    int n_frames, n_chunks;
    const FeatFrames& in;
    const FeatOut& out;
    int32_t* sel;
    bool dbg, edge;
    EdgeSel es;
};
// ---- ring_table.hip ----
// host: the ring-id table of n_rows (16 / 64) and ring_chain (SSF_RING_CHAIN_*) into out
// (ring_table_bytes); 0 or a negative code
int build_ring_table(int n_rows, int chain, void* out_host);
size_t ring_table_bytes();
// ---- launchers (feat_wave.hip, feat_chunk.hip, feat_select.hip): the single-read stage ----
// fs: the scratch this launch uses (curv_cm, irr, lmap null when it does not).  all: no
// k_feat_wave_reg ran, k_feat_wave_run takes every chunk.  launch_feat_chunk does the blocks
// flagged kIrrGeneral (fs.irr) or every block (no fs.irr).
void launch_feat_wave_reg(const FeatLaunch& a, const FeatScratch& fs);
void launch_feat_wave_run(const FeatLaunch& a, const FeatScratch& fs, bool all);
void launch_feat_chunk(const FeatLaunch& a, const FeatScratch& fs);
void launch_feat_select(const FeatLaunch& a, const FeatScratch& fs);
void launch_feat_debug(const FeatLaunch& a, const FeatScratch& fs);
// ---- launcher (feat_bin.hip): the binned stage; rtab: the ring-id table (required) ----
size_t fix_head(int n_frames);   // bytes of the fix-up lists' per-frame counts (fix_bytes)
hipError_t launch_feat_bin(const FeatLaunch& a, const BinScratch& bin, const void* rtab);

// ---- launchers (plane_table.hip) ----
hipError_t launch_plane_table(hipStream_t s, const ssf_config& cfg, int n_frames,
                              const float4* plane, const int64_t* frame_off, const int32_t* count,
                              int64_t max_m, float* normal, uint8_t* valid, float4* sorted_xyzi,
                              int32_t* sorted_idx, float4* strip_xyzi = nullptr,
                              int32_t* strip_head = nullptr);
// Point-to-line blocks of launch_register (beyond the reference; nullptr = planes only): the
// edge clouds, the last frames' line table (6 floats per edge: centroid, direction) and the
// correspondence scratch / per-pair counts.
struct EdgeReg {
    const float4* last;
    const int64_t* last_off;
    const int32_t* last_count;
    const float* line;
    const uint8_t* line_valid;
    const float4* curr;
    const int64_t* curr_off;
    const int32_t* curr_count;
    int64_t max_m;
    CorrRec* corr;
    int32_t* ncorr;
};
// The arguments of launch_register.  A caller value-initialises a RegisterArgs and fills the
// fields it has by name; a field left null is "not given".
struct RegFrames {            // the pairs' last or current plane clouds
    const float4* xyzi;
    const int64_t* off;       // per pair
    const int32_t* count;     // per pair
};
struct RegTable {             // the last frames' plane table (launch_plane_table's outputs)
    const float* normal;
    const uint8_t* valid;
    const float4* sorted;     // x-sorted copy and permutation; null: brute-force association
    const int32_t* sidx;
    const float4* strip_xyzi; // the kept strip image; null: the association builds its strips
    const int32_t* strip_head;
};
struct RegPoses {             // 7 doubles per pair (quaternion x, y, z, w, translation)
    const double* in;         // warm starts; null: rel (in place)
    const double* abs_in;     // start poses; null: abs (in place)
    double* rel;
    double* abs;              // nullable
};
struct RegOut {               // all nullable
    double* log;
    int32_t* nlog;
    int32_t* ncorr;
    int32_t* nn;
};
struct RegScratch {
    CorrRec* corr;            // >= the current frames' total points
    int32_t* nnv;             // >= the current frames' total points and
    int32_t* ncompact;        // >= n_pairs: let the lane-mode association hand the solve
                              // compacted records; null: records in query order
};
// bytes of corr, and of nnv with ncompact behind it (ncompact = nnv + reg_queries(total))
inline size_t reg_queries(int64_t total) { return (size_t)std::max<int64_t>(total, 1); }
inline size_t reg_corr_bytes(int64_t total) { return sizeof(CorrRec) * reg_queries(total); }
inline size_t reg_cidx_bytes(int64_t total, int n_pairs) { return sizeof(int32_t) * (reg_queries(total) + (size_t)n_pairs); }
struct RegisterArgs {
    RegFrames last;
    RegTable table;
    RegFrames curr;
    RegPoses pose;
    RegOut out;
    RegScratch scratch;
    int64_t max_m;            // bound of the plane points of any frame
    const EdgeReg* edge;      // null: planes only
};
// association (associate.hip), then edge association (edges.hip), then the solve (solve.hip)
hipError_t launch_register(hipStream_t s, const ssf_config& cfg, int n_pairs, const RegisterArgs& a);
// What launch_register launches for the association of n_pairs pairs bounded by max_m plane
// points, given the sorted buffers (and, for `compacted`, the nnv / ncompact scratch): host
// arithmetic only.  strips = false: not the k_associate_strips path, the other fields are 0.
struct RegisterPlan {
    bool strips;      // k_associate_strips (max_m <= the LDS sort limit)
    bool coop;        // group mode: one query per lane group, qsplit work-groups per pair
    bool soa;         // 14-B SoA staging instead of float4
    bool compacted;   // the association writes compacted records and the solve streams them in
    int qsplit;       // work-groups per pair
    int lds_cap;      // last-frame points staged in LDS (a longer last frame walks global memory)
};
RegisterPlan register_plan(int n_pairs, int64_t max_m, bool with_edges);
// launch_register's three stages, each beside its kernels (pin / ain: the resolved warm starts
// and start poses; ncp: the compacted-record counts or null); launch_register checks for errors
void launch_associate(hipStream_t s, int n_pairs, const RegisterPlan& plan, const RegisterArgs& a,
                      const double* pin);
void launch_edge_associate(hipStream_t s, int n_pairs, const EdgeReg* edge, const double* pin);
void launch_solve(hipStream_t s, const ssf_config& cfg, int n_pairs, const RegisterArgs& a,
                  const double* pin, const double* ain, int32_t* ncp);
hipError_t launch_edge_table(hipStream_t s, const ssf_edge_config& ec, int n_frames,
                             const float4* edges, const int64_t* frame_off, const int32_t* count,
                             int64_t max_m, float* line, uint8_t* valid);
hipError_t launch_accumulate(hipStream_t s, int n, const double* rel, const double* start,
                             double* abs_out);

// ---- launcher (mask_pose.hip) ----
// How a mask launch of n_frames frames (`total` points) runs and what scratch it needs: host
// arithmetic only.  G > 1 cuts every frame into G parts on G work-groups (sync: ticket +
// per-frame arrival counters; parts: exchange slots).  split: parts per frame, 0 = automatic,
// as many as keep the `slots` resident work-groups of k_mask_pose (mask_pose_slots) busy; a fixed
// split is honoured as set (frames x G may exceed the slots: work-groups then take several
// tickets) and its exchange scratch grows with it (frames x G x 104 KiB, see
// ssf_set_mask_split).  Only the GMM fit splits.  queue > 0 (G == 1, fewer than n_frames): at
// most `queue` work-groups taking frame tickets in order (the frame queue; sync holds the ticket).
struct MaskPlan {
    int G;                // parts per frame, 1 .. kMaskMaxSplit
    bool tickets;         // work-groups take (frame, part) tickets from sync: G > 1 or the queue
    int grid;             // work-groups: n_frames x G, at most slots (split) or queue
    int queue;            // the frame queue in effect, else 0
    size_t draws_bytes;   // 3 doubles per frame
    size_t rec_bytes;     // mask_rec_bytes (GMM), else 0
    size_t sync_bytes;    // with tickets, else 0
    size_t parts_bytes;   // G > 1, else 0
};
MaskPlan mask_plan(int n_frames, int64_t total, int mode, int split, int slots, int queue);
// The arguments of launch_mask_pose on storage type T (float: mask_pose.hip, double:
// mask_pose_f64.hip).  order (nullable): the dispatch order of the frames (a device permutation).
template <class T>
struct MaskArgs {
    const T* pts;
    const T* flow;
    const int64_t* frame_off;
    int mode;
    const uint8_t* mask_in;
    const double* draws;
    uint2* lloyd_rec;
    int reflection;
    uint8_t* bg_mask;
    double* out;
    uint32_t* sync;       // plan.sync_bytes
    double* parts;        // plan.parts_bytes
    const int32_t* order;
};
template <class T>
hipError_t launch_mask_pose(hipStream_t s, int n_frames, const MaskPlan& plan, const MaskArgs<T>& a);
int mask_pose_slots(int device);
// ---- launcher (kabsch_f32.hip): the float32 slove_RT_by_SVD + Quaternion tail per frame; source
// rows = dst + flow (f32) when flow is given, else src; keep_failures: leave frames whose status
// is SSF_POSE_GMM_FAILED / SSF_POSE_SYNC_FAILED (a k_mask_pose output) untouched.
hipError_t launch_kabsch_f32(hipStream_t s, int n_frames, const float* src, const float* dst,
                             const float* flow, const int64_t* frame_off, const uint8_t* mask,
                             int reflection, int keep_failures, double* out);
// ---- launcher (subsample.hip): the seeded subsample of ssf_subsample_batch, one work-group per
// frame; h_tag (host, nullable) rides in the kernel arguments.
hipError_t launch_subsample(hipStream_t s, int n_frames, const float* pts, int stride,
                            const int64_t* frame_off, const uint8_t* cls, int nb, float z_min,
                            int use_z, int quota, uint64_t seed, const uint64_t* h_tag, int key_bits,
                            int32_t* idx, float* xyz, int32_t* n_out, int32_t* status);
// ---- launchers (scan_context.hip): the Scan Context descriptor of n_clouds ragged clouds, one
// work-group per cloud; and the exhaustive comparison of n_query descriptors with candidates
// 0 .. n_cols - 1 of n_db (dist / shift rows of n_db entries, never null here) followed by the
// selection over each query's eligible prefix.  n_cols == 0 launches the selection only.
hipError_t launch_sc_describe(hipStream_t s, int n_clouds, const float* pts, int stride, const int64_t* off,
                              float max_range, float lidar_height, float* desc);
hipError_t launch_sc_match(hipStream_t s, int n_query, const float* query, int n_db, int n_cols, const float* db,
                           const int32_t* n_eligible, float* dist, int32_t* shift, ssf_sc_best* best);
// The same comparison (the same k_sc_match launch) followed by the greedy top-k selection with an
// exclusion window: best is [n_query, k], k in 1 .. SSF_SC_MAX_TOPK, exclusion >= 0.
hipError_t launch_sc_match_topk(hipStream_t s, int n_query, const float* query, int n_db, int n_cols,
                                const float* db, const int32_t* n_eligible, float* dist, int32_t* shift, int k,
                                int exclusion, ssf_sc_best* best);
size_t mask_sync_bytes(int n_frames);
size_t mask_parts_bytes(int n_frames, int G);
// The Lloyd record / queue buffer of a launch of `total` points in n_frames frames: 8-byte
// records, one per point, kLloydSpareRecs spare per frame (its even start and the spare slot
// after it) and a pair at the end; then 4-byte relabel-queue entries, one per point and
// kLloydSpareQueue spare slots per frame.  The kernel's side: mask_lloyd.hpp.
constexpr int kLloydSpareRecs = 2;
constexpr int kLloydSpareQueue = 64;
constexpr int64_t lloyd_rec_count(int64_t total, int n_frames) { return total + kLloydSpareRecs * (int64_t)n_frames + 2; }
constexpr int64_t lloyd_queue_count(int64_t total, int n_frames) { return total + kLloydSpareQueue * (int64_t)n_frames; }
size_t mask_rec_bytes(int64_t total, int n_frames);

// ---- launchers (loop.hip) ----
struct IcpState {             // one per ICP problem, device-resident across iterations
    float fin[16];            // final transformation (row-major, float as PCL's Matrix4f)
    double prev_mse;
    double fitness;
    int32_t it, done, state, converged, n_corr, pad;
};
typedef ssf_icp_params IcpParams;
size_t vg_scratch_bytes(int n_clouds, int64_t n);
hipError_t launch_voxel_grid(hipStream_t s, int n_clouds, const float4* pts, const int64_t* off,
                             int64_t n, int64_t max_pts, float leaf, void* scratch, float4* out,
                             int32_t* out_count);
// clouds [off[c], off[c + 1]) of in -> out at the same offsets, cloud c by the 12 doubles at
// T + 12 c; base = off[0], total = off[n_clouds] - off[0] (host values)
hipError_t launch_transform_clouds(hipStream_t s, int n_clouds, const float4* in, const int64_t* off,
                                   int64_t base, int64_t total, const double* T, float4* out);
hipError_t launch_icp_init(hipStream_t s, int n_prob, const float4* src, const int64_t* soff,
                           int64_t max_ns, const float* guess, float4* cur, IcpState* st,
                           unsigned long long* key);
hipError_t launch_icp_iteration(hipStream_t s, int n_prob, float4* cur, const int64_t* soff,
                                int64_t max_ns, const float4* tgt, const int64_t* toff,
                                int64_t max_nt, const IcpParams& prm, IcpState* st,
                                unsigned long long* key);
hipError_t launch_icp_fitness(hipStream_t s, int n_prob, const float4* src, const int64_t* soff,
                              int64_t total_ns, int64_t max_ns, const float4* tgt,
                              const int64_t* toff, int64_t max_nt, IcpState* st,
                              unsigned long long* key);

// ---- launcher (pose_graph.hip) ----
struct PgoGraph {             // one per graph, built on the host from the host offsets
    int64_t scratch_off;      // this graph's piece of the context scratch, in doubles
    int32_t node0, K, edge0, E;
    int32_t lcap;             // min(max(E - (K - 1), 0), SSF_PGO_MAX_LOOPS): loop edges it has room for
    int32_t wide;             // pgo_graph_wide(K, E): solved by k_pose_graph_wide
};
bool pgo_graph_wide(int K, int E);      // more than 32 edges beyond K - 1: it may hold more than 32 loops
size_t pgo_graph_doubles(int K, int E, int lcap, bool wide, bool lm);   // lm: with the trial buffers
// The arguments of the pose-graph kernels, passed to them by value; value-initialise, then set
// (device pointers unless noted).  The first 14 are every kernel's.
struct PgoArgs {
    const PgoGraph* desc;
    double* pose;
    const int32_t* node_off;
    const int32_t* edge_ij;
    const double* edge_meas;
    const double* edge_var;
    const int32_t* edge_off;
    const double* prior_pose;
    const double* prior_var;
    int max_iter;
    double func_tol;
    double* scratch;          // sized by pgo_graph_doubles, with lm = has_lm
    double* stats;
    double* cost_log;         // nullable
    // the kernels with a loss (ssf_pgo_robust: rkind, rk) on the loop edges
    int rkind;
    double rk;
    double* edge_out;         // nullable
    // the loss kernels with step control
    ssf_pgo_lm lm;
    double* lm_log;           // nullable
    // which kernel pair (host only): has_lm the step-control kernels, else robust the loss
    // kernels, else the plain ones
    bool robust, has_lm;
};
hipError_t launch_pose_graph(hipStream_t s, int n_graphs, bool any_narrow, bool any_wide, const PgoArgs& a);

}  // namespace ssf
