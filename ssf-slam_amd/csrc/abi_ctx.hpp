// abi_ctx.hpp -- what the extern "C" entry points of libssf_frontend.so (include/ssf_frontend.h,
// the abi_*.hip files) share: the context with its device scratch, the kernel timer and the
// error helpers.
//
// Host side of the boundary: argument checks, per-context device scratch (grown on demand,
// never shrunk; ssf_reserve pre-sizes it), the numpy-legacy RandomState used by the GMM
// k-means++ init, and kernel launches on the caller's stream.  No C++ exception crosses the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "numpy_rng.hpp"
#include "ssf_internal.hpp"

using ssf::DevBuf;

// Kernel timing (ssf_profile_enable): events recorded on the launching stream right before each
// kernel and at the end of the ABI call; consecutive events bracket one kernel.  On a stream
// that no other stream competes with, that is the kernel's own duration.
struct KTimer {
    bool on = false;
    struct Mark { hipEvent_t ev; const char* name; };   // name == nullptr closes an ABI call
    std::vector<Mark> marks;
    std::vector<hipEvent_t> pool;                       // events reused after every read
    static constexpr size_t kMaxMarks = 1 << 14;
    static thread_local KTimer* current;                // the timer of the ABI call running on this thread (abi_core.hip)
    void mark(hipStream_t s, const char* name) {
        if (marks.size() >= kMaxMarks) return;          // unread backlog: stop recording
        if (marks.size() == pool.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return;
            pool.push_back(e);
        }
        hipEvent_t e = pool[marks.size()];
        if (hipEventRecord(e, s) != hipSuccess) return;
        marks.push_back({e, name});
    }
    ~KTimer() {                                         // ssf_destroy has waited for the last mark
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
};

// The context owns its scratch: every member releases itself when ssf_destroy deletes the
// context, so no function lists the buffers.  Members are destroyed in reverse declaration
// order, which the teardown relies on: the draw slots, declared after every plain buffer, go
// first (each waits for its events), the timer's events, declared before them, go last.
struct ssf_ctx {
    int device = 0;
    ssf_config cfg{};
    std::string err;
    KTimer prof;
    // frameFeature scratch
    DevBuf rid, hist, ring_off, ring_xyzi /* ring index */, sel, sel_cnt /* candidate flags */, fix, plane1, off1, cnt1;
    // single-read feature stage: per-(chunk, row) counts, u16 chunk positions, bit planes,
    // chunk-major curvature (debug outputs only)
    DevBuf fcnt, fidx, fbits, fcurv, rtab, firr, flmap;
    bool rtab_ready = false;
    // registration scratch
    DevBuf corr;
    DevBuf cidx;                       // compacted-record scratch: per query (index, valid), per pair count
    // ssf_register_pair: offsets, counts, the last frame's plane table + search index, pose, log
    DevBuf pair;
    DevBuf start1;                     // ssf_accumulate_sequence: the start pose
    // edge features (beyond the reference): selection scratch, correspondence records
    ssf_edge_config ecfg{};
    DevBuf esel, ecorr;
    // loop closure (loop.hip): voxel-grid sort scratch; ICP transformed source, 1-NN keys,
    // per-problem state and guesses
    DevBuf vg, icp_cur, icp_key, icp_st, icp_guess;
    // pose graph (pose_graph.hip): per-graph descriptors (host copy reused across calls) and the
    // working poses, factor records, block factors and right-hand sides of every graph
    DevBuf pgo_desc, pgo_scratch;
    std::vector<ssf::PgoGraph> pgo_h;
    // scan context (scan_context.hip): the dist / shift rows of a selection-only match
    DevBuf sc_rows;
    ssf::NumpyRandomState rng;         // host RandomState of the k-means++ draws
    int mask_split = 0;                // ssf_set_mask_split: 0 = automatic
    const int32_t* mask_order = nullptr;   // ssf_set_mask_schedule
    int mask_order_n = 0, mask_queue = 0;
    int mask_slots = -1;               // resident k_mask_pose work-groups (queried once: slots())
    int slots() {
        if (mask_slots < 0) mask_slots = ssf::mask_pose_slots(device);
        return mask_slots;
    }
    // mask: k-means++ draws staged per launch through a ring of slots, so launches on different
    // streams (e.g. consecutive batches overlapping their slow frames) never share a buffer
    struct DrawSlot {
        DevBuf d;
        DevBuf rec;                    // Lloyd label/bound records (8 B) + relabel queue (4 B) per point
        DevBuf sync, parts;            // frame split: ticket + arrival counters, exchange slots
        double* h = nullptr;           // pinned staging
        int64_t hcap = 0;
        hipEvent_t copied = nullptr;   // this slot's H2D finished: the staging may be rewritten
        hipEvent_t used = nullptr;     // the kernel that read this slot finished
        ~DrawSlot() {                  // wait for the slot's last launch, then the buffers go
            if (used) { (void)hipEventSynchronize(used); (void)hipEventDestroy(used); }
            if (copied) { (void)hipEventSynchronize(copied); (void)hipEventDestroy(copied); }
            if (h) (void)hipHostFree(h);
        }
    };
    static constexpr int kDrawSlots = 4;
    int dnext = 0;
    DrawSlot dslot[kDrawSlots];        // declared last: torn down first
};

// Scope of one ABI call: its launches mark into the context's timer when timing is on.
struct ProfScope {
    KTimer* prev;
    KTimer* mine;
    hipStream_t s;
    ProfScope(ssf_ctx* c, void* stream)
        : prev(KTimer::current), mine(c && c->prof.on ? &c->prof : nullptr), s((hipStream_t)stream) {
        if (mine) KTimer::current = mine;
    }
    ~ProfScope() {
        if (mine) { mine->mark(s, nullptr); KTimer::current = prev; }
    }
};

inline int32_t fail(ssf_ctx* c, int32_t code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

inline int32_t hip_fail(ssf_ctx* c, hipError_t e, const char* where) {
    if (c) c->err = std::string(where) + ": " + hipGetErrorString(e);
    return SSF_E_HIP;
}

// the return code of the HIP call (a launcher, mostly) that ends an entry point
inline int32_t hip_rc(ssf_ctx* c, hipError_t e, const char* where) {
    return e == hipSuccess ? SSF_OK : hip_fail(c, e, where);
}

#define SSF_TRY_HIP(ctx, expr, where)                              \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return hip_fail((ctx), _e, (where)); \
    } while (0)

// A table's strip image comes with both of its buffers and with the sorted buffers; who fails
// the check prefixes the message with its name.
inline bool strip_args_ok(const void* strip_xyzi, const void* strip_head, const void* sorted_xyzi,
                          const void* sorted_idx) {
    return !strip_xyzi == !strip_head && (!strip_xyzi || (sorted_xyzi && sorted_idx));
}
constexpr const char* kStripArgsMsg = ": the strip image needs both strip buffers and the sorted buffers";

// abi_features.hip: the feature scratch of n_frames frames (ssf_reserve pre-sizes with it)
int32_t ensure_features(ssf_ctx* c, int32_t n_frames, int64_t total, int64_t max_pts);
