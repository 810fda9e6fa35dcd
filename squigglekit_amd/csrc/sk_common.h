// sk_common.h -- internal declarations shared by the HIP translation units.
// gfx950 only.  Not part of the public ABI (that is include/squigglekit_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdarg.h>
#include <vector>
#include "squigglekit_hip.h"

#define SK_MAX_DEVICES 16
#define SK_WAVE 64

// Per-read result of the prep kernel; consumed by the DTW / segment kernels.
// 48 bytes, one per read, lives in HBM.
struct sk_prep {
    int32_t n;        // samples surviving scale_outliers
    int32_t flags;    // SK_FLAG_*
    double  center;   // medmad: median            zscale: mean       segmenter: median
    double  scale;    // medmad: MAD*1.4826        zscale: std (0->1) segmenter: std
    double  top;      // segmenter: median + std*std_scale   (segmenter.py:413)
    double  bot;      // segmenter: median - std*std_scale   (segmenter.py:414)
};

// Internal flag bits of sk_prep::flags (never reach sk_hit::flags: the DTW kernels keep the low byte only).
// INPLACE: nothing of this float64 read was dropped by the filter, so its filtered samples were not copied -- the DTW
// feed reads them from the caller's buffer (sk_sdtw_args::samples_raw) at the same offsets.
#define SK_IFLAG_INPLACE 0x100
#define SK_FLAG_PUBLIC   0xff

enum sk_prep_mode { SK_PREP_MEDMAD = 0, SK_PREP_ZSCALE = 1, SK_PREP_SEGMENT = 2, SK_PREP_DRNA = 3 };

// which statistics route wrote sk_ctx::redo (sk_last_f64_retries / sk_last_pa_retries)
enum sk_redo_route { SK_REDO_NONE = 0, SK_REDO_I16 = 1, SK_REDO_F64 = 2, SK_REDO_PA = 3 };

// Growable device scratch buffer.
struct sk_buf {
    void  *p = nullptr;
    size_t cap = 0;
};

// Motif panel (sk_panel.hip): one motif's place in the per-call device table, and the motifs that share a lane layout.
struct sk_panel_motif {
    int32_t xoff;     // first double of its [L][R] layout inside the panel's layout block
    int32_t P;        // short lanes (own R - 1 rows)
    int32_t k;        // the caller's motif index: records go to out[k * out_stride + read]
    int32_t pad;
};
struct sk_panel_group {
    int32_t L, R;     // lanes per read, rows per lane
    int32_t first, count;   // its run of table entries
};

// DTW over a pair list (sk_pairs.hip): what one lane group of a launch reads from the per-call device table.  32 bytes.
struct sk_pair_entry {
    int64_t toff;     // first sample of the target inside the pool
    int64_t xoff;     // first double of the query's [L][R] layout inside the call's layout block
    int32_t n;        // the target's length
    int32_t P;        // the query's short lanes (own R - 1 rows)
    int32_t pair;     // the caller's pair index: the record goes to out[pair]
    int32_t pad;
};
// ... and one distinct query of the call: where its points lie in the pool, where its layout goes (k_pairs_layout)
struct sk_pair_query {
    int64_t src, xoff;
    int32_t N, L, R, pad;
};

// Mapping sessions (sk_mapstream.hip): what one lane group of a MODE_PAIRS_CHAIN launch reads -- a table type of its own,
// so that sk_pair_entry and the code that reads it stay as they are.  48 bytes.
struct sk_map_entry {
    int64_t toff;     // first point of the target inside the session's target pool
    int64_t xoff;     // first double of the chunk piece's [L][R] layout inside the push's layout block
    int64_t soff;     // first column of this (slot, target)'s row state inside the session's D / S arrays
    int32_t n;        // the target's length (>= 1)
    int32_t P;        // the piece's short lanes (own R - 1 rows)
    int32_t rec;      // the record goes to last[rec] (slot * ntargets + target)
    int32_t cont;     // 0: fresh, the virtual row -1 enters (MODE_PAIRS); 1: continuing, the stored row enters (MODE_CHAIN)
};

// Hit lists over a pair list / a mapping session (sk_pairhits.hip): one last row of the select's table.  24 bytes.
struct sk_rowhit_entry {
    int64_t col0;     // first column of the row inside the D and S arrays
    int64_t list;     // its K records go to out[list * K ..], its count to count[list]
    int32_t n;        // columns (the target's length)
    int32_t flags;    // SK_FLAG_* of the records, | SK_ROWHIT_NOROW
};
#define SK_ROWHIT_NOROW 0x100   // internal (never reaches sk_hit::flags): no row is stored -- count 0, nothing is read

// ... and one pair of a paths call over the list (sk_pairpath.hip): where its query and target lie in the pool, their
// lengths, the first row of its spans.  32 bytes.
struct sk_pairpath_entry {
    int64_t qoff, toff;   // first point of the query / of the target inside the pool
    int64_t span_off;     // first row of the pair's spans: the query lengths of the pairs before it, summed
    int32_t N, M;         // the query's and the target's length
};

// ... and one pair of an adaptive-band call (sk_band.hip): the same places and lengths, and the caller's pair index (the
// table is ordered longest N + M first; records go to out[pair]).  40 bytes.
struct sk_band_entry {
    int64_t qoff, toff;
    int64_t span_off;
    int32_t N, M;
    int32_t pair, pad;
};

struct sk_ctx {
    int         device = -1;
    bool        ready = false;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;    // second stream (created on first use): overlapped walks / copies
    hipStream_t stream3 = nullptr;    // third stream (created on first use): the early exact retry beside the window passes
    hipEvent_t  ev_r[2] = {nullptr, nullptr};   // its ordering events: pass Q done / early retry done
    hipStream_t stream4 = nullptr;    // fourth stream (created on first use): the audit's exact sweep beside the window passes
    hipEvent_t  ev_a = nullptr;       // audit sweep done
    hipEvent_t  ev_s[2] = {nullptr, nullptr};   // second clusters (siblings) on the third stream: pass Q done / their round done
    uint32_t    dtw_sparse_calls = 0; // calls whose audit would be exposed (few, long reads): every K-th is audited
    uint32_t    dtw_audit_calls = 0;  // audited launches so far: salt of the audit's choice of reads (k_audit_pick)
    hipEvent_t  ev_chunk[9] = {};     // ordering events between the two streams (no timing)
    hipEvent_t  ev[4] = {nullptr, nullptr, nullptr, nullptr};   // prep start/stop, main start/stop
    bool        ev_valid = false;
    int         num_cu = 0;
    // scratch (grown on demand, reused across calls)
    sk_buf sig;       // staged input samples
    sk_buf len;       // int32 per read
    sk_buf rlen;      // int32 per read: the caller's per-read cut of a ragged float64 batch (sk_segment_batch_f64_len)
    sk_buf off;       // int64 per read (+1) for ragged f64
    sk_buf comp;      // compacted samples
    sk_buf prep;      // sk_prep per read
    sk_buf mask;      // in-band bit masks (segmenter)
    sk_buf motif;     // laid-out motif rows
    sk_buf out;       // sk_hit / segs staging
    sk_buf out2;      // nsegs staging
    sk_buf misc;
    sk_buf seghints;  // per read: the stretches of quiet mask entries and their anchors, k_seg_stats -> k_seg_walk4
    sk_buf pacal;     // per read {offset, range / digitisation}: the pA conversion of raw rows (sk_segment_batch_i16_pa)
    sk_buf pull;      // SquigglePull text: tile / line scans (int64) and the error word (sk_pull.hip)
    sk_buf pulltext;  // SquigglePull text: the prefixes and the text of the host entry point
    sk_buf sweep;     // parameter sweep: the sets in walk form, then the summaries (sk_sweep.hip)
    sk_buf sweeprec;  // parameter sweep: the per-(set, read) records of the host entry points
    sk_buf hitrows;   // hit lists: the last rows of a chunk of reads (cost f64, start i32) and their records
    sk_buf bgrec;     // read background: the sk_bg_rec [nmotifs][nreads] of the host entry points
    sk_buf pathcnt;   // alignment paths: [0] = hits of the call that failed the self-check (sk_last_path_mismatches)
    bool   path_valid = false;   // ... set by the first paths / events call (sk_path_begin) and never cleared: the counter is
                                 // the last such call's, also after a later call that makes no paths
    sk_buf pathlist;  // alignment paths: [0] = count, [2 ..] = hits of a launch left to the scratch tier
    sk_buf pathscratch;   // alignment paths: the scratch tier's slabs (direction words + stripe boundary row per wavefront)
    sk_buf pathmotif; // alignment paths: the motifs of the call, flat (device)
    sk_buf pathspans; // alignment paths: the spans of the host entry points
    sk_buf events;    // events: the sk_event records of the host entry points
    sk_buf poolev;    // events: the records sk_events_pool uploads
    sk_buf pool;      // events: pooling scratch -- the result [N], the count, the mask, the list of selected hits
    sk_buf panel;     // motif panel: the motifs of the call laid out per lane, their table, mean / sd (sk_panel.hip)
    sk_buf panelwin;  // motif panel: the window rows (int16, stride wstride) or the gathered float64 windows
    sk_buf panelaux;  // motif panel: per read window length, resolved begin, the caller's win rows / float64 offsets
    sk_buf panelrec;  // motif panel: [K][R] records when the caller takes none, and the host entry points' sk_panel_rec
    sk_buf seglev;    // segment levels: the sk_seg_level records of the host entry points ([nreads][max_segs], then [nreads])
    sk_buf seglevwork;    // segment levels: [0] = items, [4 ..] = the (read, slot) work list, then the long items' scratch rows
    sk_buf detect;    // event detection: the mark words [nreads][ceil(stride / 64)], then the scan's block sums (sk_detect.hip)
    sk_buf detectout; // event detection: off [nreads + 1], then the sk_det_event records of the host entry point
    sk_buf hmm;       // signal HMM: the sk_hmm_rec records of the host entry points, then their {offset, unit} pairs (sk_hmm.hip)
    sk_buf hmmpath;   // state paths: a slice's back pointers [group][t][lane], its segment counts, the scan's block sums
    sk_buf hmmseg;    // state paths: off [nreads + 1], then the sk_hmm_seg records of the host entry points
    sk_buf hmmpost;   // posteriors: a slice's L, checkpoints [group][block][state][lane] and slabs (sk_hmm_post.hip)
    sk_buf hmmpostout; // posteriors: counts, goff and dense rows of the host entry points
    std::vector<double> panel_host;           // laid-out motifs as uploaded (kept alive for the async H2D)
    std::vector<sk_panel_motif> panel_table;  // one entry per motif of at most 1 024 points, group after group
    std::vector<sk_panel_group> panel_groups;
    std::vector<int32_t> panel_long;          // motifs of more than 1 024 points: the chained launcher, one at a time
    sk_buf pairs;     // pair list: the distinct queries laid out per lane, then the table (sk_pairs.hip)
    sk_buf pairsval;  // pair list: the pool and the records of the host entry point
    std::vector<sk_pair_query> pairs_query;   // one entry per distinct query (kept alive for the async H2D)
    std::vector<sk_pair_entry> pairs_table;   // one entry per pair, (L, R) group after group
    sk_buf rowhit;    // pair / session hit lists: the select's table, one sk_rowhit_entry per row (sk_pairhits.hip)
    std::vector<sk_rowhit_entry> rowhit_table;       // (kept alive for the async H2D)
    std::vector<sk_map_entry>    pairhits_sweep;     // pair hit lists: the sweep's entries, slice after slice (kept alive likewise)
    int64_t pairhits_row_bytes = 0, pairhits_slices = 0, pairhits_long_rows = 0;   // the last such call (sk_last_pair_hits_plan)
    sk_buf pairpath;  // pair-list paths: the table, one sk_pairpath_entry per pair (sk_pairpath.hip)
    std::vector<sk_pairpath_entry> pairpath_table;   // (kept alive for the async H2D)
    int64_t pairpath_listed = 0, pairpath_slab_bytes = 0, pairpath_waves = 0;   // the last such call: pairs left to the
                                                                                 // scratch tier, bytes of a slab, wavefronts
    sk_buf band;      // adaptive-band DTW: the table, one sk_band_entry per pair (sk_band.hip)
    sk_buf bandslab;  // ... the wavefronts' slabs: direction words, then move bits
    std::vector<sk_band_entry> band_table;    // (kept alive for the async H2D)
    int64_t band_slab_bytes = 0, band_waves = 0, band_steps = 0;   // the last such call (sk_last_band_plan)
    sk_buf ckpt;      // DTW checkpoints (systolic state dumps: doubles or fixed-point units)
    sk_buf motifq;    // fixed-point motif layout
    sk_buf motif64;   // the motif laid out for 64 lanes (retry pass of a short motif)
    bool   motif64_valid = false;
    std::vector<double> motif64_host;
    sk_buf lastq;     // screening pass: last-row costs per column
    sk_buf qflag;     // screening pass: per-read "left the fixed-point range" flags
    sk_buf wsoft;     // window pass: reads of the chunk that go to its second tier ([0] = count)
    sk_buf lsum;      // screening pass: last-row minima per checkpoint interval and lane
    sk_buf wstate;    // window pass: restart state per read (pass P -> pass W)
    sk_buf wrec;      // window pass: restart point per read {tbase, jlo, jhi, flags}
    sk_buf wrecq;     // screening pass epilogue: candidate columns per read (first tier of pass P)
    sk_buf order;     // [1024] sort cursors, then the chunk's reads in the order the window passes take them
    sk_buf motifw;    // the motif (doubles) in the screening scheme's own per-lane layout
    std::vector<double> motifw_host;
    int    motifq_L = 0;   // lanes per read of the layouts in motifq / motifw
    sk_buf retry;     // DTW retry list: [0] = count, [1] = pad, [2 ..] = reads
    sk_buf dtwcnt;    // [0] = reads retried by the exact pass, summed over the launches of one API call (device); [1] second tier; +16 clock; +32 guard counters
    sk_buf audit;     // the audit's read list ([0] = count, [2 ..] = reads) and its exact records
    sk_buf sib;       // window passes: [0..3] count, then {read, jlo, jhi, -} per second cluster of candidate columns
    sk_buf sibout;    // ... and pass W's record per sibling
    sk_buf sibstate;  // ... their own pass-P state and window records (the round runs beside the main window passes)
    bool   retry_dev = false;   // the last DTW call left its retry count on the device (read lazily)
    std::vector<unsigned> motifq_host;
    bool   motifq_valid = false;
    // numpy-order redo lists of the segmenter's statistics routes (int16, float64, pA): a buffer of their own, so that
    // no DTW launch moves or overwrites them.  Per list [0] = count, [1 ..] = reads; the lists of one API call (one
    // per sub-batch) lie side by side.  redo_route: the route that wrote them in the last MotifSeq / segmenter call,
    // redo_off: where in `redo` the counters of that call are (ints), redo_used: ints handed out so far in that call.
    sk_buf redo;
    int    redo_route = SK_REDO_NONE;
    std::vector<size_t> redo_off;
    size_t redo_used = 0;
    std::vector<int64_t> pa_off_host;             // slot offsets of the float64 fallback of the pA route
    int    last_retry = 0;   // reads that needed the exact single-pass retry in the last DTW call
    std::vector<hipEvent_t> evpool;   // per-launch events of the two-pass DTW (3 per chunk)
    int    prof_chunks = 0;  // chunks of the last two-pass DTW call (0: single pass)
    int    prof_reads[64] = {0};
    std::vector<double> motif_host;   // last laid-out motif (kept alive for async H2D)
    std::vector<double> motif_src;    // the motif it was built from (upload cache key, with motif_L)
    int    motif_L = 0;               // lanes per read of the layout in `motif`
    void  *comm = nullptr;            // ncclComm_t of this device (sk_comm.hip), or nullptr
    void  *sessions[SK_STREAM_MAX_SESSIONS] = {};   // MotifSeq sessions of this context (sk_stream.hip), by handle
    void  *map_sessions[SK_MAP_MAX_SESSIONS] = {};  // mapping sessions of this context (sk_mapstream.hip), by handle
    int64_t map_state_bytes = 0, map_entries = 0, map_launches = 0;   // the last push of one (sk_last_map_plan)
    void  *evs_sessions[SK_EVS_MAX_SESSIONS] = {};  // event sessions of this context (sk_evstream.hip), by handle
    sk_buf evscnt;                    // ... [0] = slots their pushes stopped at a guard since the context was set up (sk_last_evs_plan)
    int64_t evs_state_bytes = 0, evs_staged = 0;    // the last push of one: bytes of slot state, staging rows
    bool   evs_valid = false;         // a push has been made on this context (the counter is meaningful)
    void  *hmms_sessions[SK_HMMS_MAX_SESSIONS] = {};   // HMM sessions of this context (sk_hmmstream.hip), by handle
    sk_buf hmmscnt;                   // ... [0] = slots their pushes met full since the context was set up (sk_last_hmms_plan)
    int64_t hmms_state_bytes = 0;     // the last push of one: bytes of slot state
    bool   hmms_valid = false;        // a push has been made on this context (the counter is meaningful)
    void  *live_sessions[SK_LIVE_MAX_SESSIONS] = {};   // live mapping sessions of this context (sk_live.hip), by handle
    int64_t live_state_bytes = 0, live_levels = 0, live_launches = 0;   // the last push of one (sk_last_live_plan)
    sk_buf commbuf;                   // staging for the small host-side exchanges
    sk_buf pile;      // reference pile-up: counters, target offsets, row pairs, offsets, cursors, chunk table (sk_pileup.hip)
    sk_buf pileent;   // ... the inverted index's rows, 4 bytes per entry
    sk_buf pilealt;   // ... the long tier's second copy of them (merge passes go back and forth)
    sk_buf pilein;    // ... the inputs of the host entry point
    sk_buf pileout;   // ... and its records
    int64_t pile_entries = 0, pile_longest = 0, pile_long_lists = 0, pile_scratch_bytes = 0;   // the last such call (sk_last_pileup_plan)
};

// ---- tuning switches (sk_runtime.hip) ----
// Every environment switch the library reads is listed in ONE table (SK_TUNABLES in sk_runtime.hip, exported as text by
// sk_tunables()); none changes results.  They are read only when SK_TUNING=1 is set as well (tests, tools/, bench.py
// set it): a stray SK_* variable in a user's shell cannot move a production job onto a slow or rarely used path.
// sk_tune() returns the variable's value, or nullptr when it is unset, tuning is off, or the name is not in the table.
const char *sk_tune(const char *name);

// ---- runtime (sk_runtime.hip) ----
// Every public entry point that touches a context opens with an sk_entry and holds it to its return (SURVEY 8(b):
// "per-device context guarded by a mutex"): it takes the slot's lock first, then checks that the context is ready
// (SK_ERR_NO_DEVICE otherwise: never set up, or shut down while this thread waited for the lock), then makes its
// device current.  Two host threads bound to the same slot take turns call by call -- the scratch buffers sk_reserve
// may free, the streams' event slots and the "last call" counters belong to one call at a time.  Contexts of different
// slots never wait for each other; g_mu (sk_init_slot, sk_shutdown) is always taken before a context lock.
struct sk_entry {
    sk_ctx *c = nullptr;                     // nullptr: no ready context (the error is set)
    sk_entry();                              // the slot the calling thread is bound to
    explicit sk_entry(int slot);
    ~sk_entry();
    sk_entry(const sk_entry &) = delete;
    sk_entry &operator=(const sk_entry &) = delete;
};
#define SK_ENTER(c)                                                                     \
    sk_entry c##_entry_;                                                                \
    sk_ctx *const c = c##_entry_.c;                                                     \
    if (!c) return SK_ERR_NO_DEVICE
sk_ctx *sk_ctx_of(int device);              // context slot of a device (ready or not)
int  sk_bound_device(void);                 // device the calling thread is bound to, or -1
int  sk_fail(int code, const char *fmt, ...);
int  sk_reserve(sk_ctx *c, sk_buf *b, size_t bytes);
int  sk_second_stream(sk_ctx *c);           // creates stream2 and its ordering events ev_chunk on first use
// Reads per chunk of a checkpointing DTW call: scratch budget (64 GB, or SK_DTW_SCRATCH_MB) / per_read, at
// least 1024 reads (64 when the budget was set by hand, so that tests can force many small chunks).
int64_t sk_dtw_chunk_reads(size_t per_read, int64_t nreads);
void    sk_dtw_scratch_shrink(int reset);   // halve the calling thread's scratch budget (reset != 0: back to the default)
#define SK_HIP(call)                                                                    \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess)                                                           \
            return sk_fail(SK_ERR_HIP, "%s failed: %s (%s:%d)", #call,                 \
                           hipGetErrorString(e_), __FILE__, __LINE__);                  \
    } while (0)

// ---- prep (sk_prep.hip) ----
// i16: rows of `stride` samples; comp gets the filtered samples of read r at
// comp + r*stride.  mask (dRNA mode) gets ceil(stride/64) transposed words per read, word wi of read r at
// [wi * mask_stride + r].  SEGMENT mode writes d_mask2 instead: {in band, kept} entries in raw coordinates, row16 per
// read, entries [0, ceil(len/64)) in full (the layout sk_launch_seg_walk_masks reads).
int sk_launch_prep_i16(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len,
                       int32_t nreads, int32_t lo, int32_t hi, int mode, double std_scale,
                       int16_t *d_comp, sk_prep *d_prep, uint64_t *d_mask, int64_t mask_stride,
                       int32_t t0 = 0, int32_t t1 = 0x7fffffff,    // statistics window (filtered index)
                       // SEGMENT mode over a device-side list of reads (d_list[0 .. *d_count)): statistics in numpy's
                       // order for those reads only (the streaming segmenter's uncertified reads, sk_segstat.hip)
                       const int32_t *d_list = nullptr, const int32_t *d_count = nullptr,
                       void *d_mask2 = nullptr, int row16 = 0);
// wavefront-per-read medmad variant (sk_prepw.hip): same results; returns 1 (nothing launched) when
// the configuration is outside its range and the caller has to use the workgroup-per-read kernel
int sk_launch_prepw_medmad(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len,
                           int32_t nreads, int32_t lo, int32_t hi, int16_t *d_comp, sk_prep *d_prep);
// f64 ragged: read r is sig[off[r]..off[r+1]); comp uses the same offsets.  SEGMENT mode writes {in band, kept}
// entries in raw coordinates (row16 per read, as sk_launch_prep_i16) and each read's raw length to d_len_out.
int sk_launch_prep_f64(sk_ctx *c, const double *d_sig, const int64_t *d_off, int32_t nreads,
                       double lo, double hi, int mode, double std_scale,
                       double *d_comp, sk_prep *d_prep, void *d_mask2 = nullptr, int row16 = 0,
                       int32_t *d_len_out = nullptr,
                       const int32_t *d_rlen = nullptr);   // optional: read r is its first d_rlen[r] samples

// ---- DTW (sk_sdtw.hip) ----
// Input kinds for the sample feed.
enum sk_feed { SK_FEED_I16 = 0,      // int16 filtered samples + (center, scale) from sk_prep
               SK_FEED_F64_NORM = 1, // float64 filtered samples + (center, scale) from sk_prep
               SK_FEED_F64_RAW = 2 };// float64 already normalised (mlpy boundary), ragged
// int16 MotifSeq calls with medmad: filter + statistics can run as the prologue of the screening pass
// (sk_sdtwq.hip) instead of as a kernel of their own; sk_launch_sdtw falls back to the kernel when its
// screening scheme does not apply to the call.
struct sk_prep_fuse {
    const int16_t *raw = nullptr;   // device, rows of `stride` samples (sk_sdtw_args::stride)
    const int32_t *len = nullptr;   // device
    int32_t lo = 0, hi = 0;         // scale_outliers limits
    int     mode = SK_PREP_MEDMAD;  // SK_PREP_MEDMAD or SK_PREP_ZSCALE (round 5: reads of up to 4 096 samples)
};
// can filter + statistics of this call ride in the screening pass?  medmad: limits inside the prologue's histogram
// range; zscale: rows of at most 4 096 samples (the wave keeps the compacted read in LDS)
bool sk_sdtw_fuse_ok(int32_t lo, int32_t hi, int mode = SK_PREP_MEDMAD, int64_t stride = 0);

struct sk_sdtw_args {
    int           feed;
    const void   *samples;     // int16* or double*
    int64_t       stride;      // row stride (feed I16), ignored when off != nullptr
    const int64_t *off;        // ragged offsets (nreads+1) or nullptr
    const sk_prep *prep;       // per-read n/center/scale (nullptr for F64_RAW: n from off)
    int32_t       nreads;
    const double *motif;       // HOST pointer, nmotif points
    int32_t       nmotif;
    sk_hit       *out;         // device, nreads records
    double       *last_row;    // device, optional: cost[-1,:] of read 0 (single-pair call)
    int64_t       max_len;     // upper bound of any read's filtered length (chooses 1 vs 2 passes)
    int           force_single;// 1: always the single FULL pass
    int           accumulate = 0;  // 1: a further launch set of the same API call (keep the retry total)
    const void   *samples_raw = nullptr;  // float64 feeds: the unfiltered input (same offsets), read instead of `samples`
                                          // for reads flagged SK_IFLAG_INPLACE
    const sk_prep_fuse *fuse = nullptr;   // non-null: samples / prep are NOT filled yet (see sk_prep_fuse); they are
                                          // the writable c->comp / c->prep buffers
};
int sk_launch_sdtw(sk_ctx *c, const sk_sdtw_args *a);
// (L, R) -- lanes per read, rows per lane -- of the exact single pass for a motif of N <= 1 024 points when `count` reads
// (or (read, motif) pairs, or session slots) are swept at a time.  Every exact sweep takes its shape from here.
void sk_exact_shape(int N, int64_t count, int *L, int *R);
// the exact single pass over the `count` motifs of one (L, R) group of a panel in one grid (k_sdtw, MODE_PANEL): d_xlay
// the panel's layouts, d_mt the group's table entries, motif k's record of read r -> d_all[k * out_stride + r]
int sk_launch_sdtw_panel(sk_ctx *c, const sk_sdtw_args *a, int L, int R, const double *d_xlay, const sk_panel_motif *d_mt,
                         int32_t count, sk_hit *d_all, int64_t out_stride);
// the exact single pass over `count` pairs of one (L, R) group of a pair list in one grid (k_sdtw, MODE_PAIRS; global != 0:
// MODE_PAIRS_GLOBAL): lane group g reads d_pt[g] -- its query's layout inside d_xlay, its target inside d_values, its
// pair index -- and writes d_out[pair]
int sk_launch_sdtw_pairs(sk_ctx *c, int L, int R, int global, const double *d_values, const double *d_xlay,
                         const sk_pair_entry *d_pt, int32_t count, sk_hit *d_out);
// ... and over `count` (chunk piece, target) entries of one (L, R) group of a mapping session's push (k_sdtw,
// MODE_PAIRS_CHAIN): lane group g reads d_mp[g], sweeps its piece over its target -- fresh or continuing from the row state
// at stD / stS + soff -- stores the new last row there and writes d_last[rec]
int sk_launch_sdtw_map(sk_ctx *c, int L, int R, const double *d_targets, const double *d_xlay, const sk_map_entry *d_mp,
                       int32_t count, double *stD, int32_t *stS, sk_hit *d_last);
// k_pairs_layout over nq distinct queries (sk_pairs.hip): d_qt[i]'s points from d_values into its per-lane layout in d_lay
int sk_launch_pairs_layout(sk_ctx *c, const double *d_values, const sk_pair_query *d_qt, int nq, double *d_lay);
// the plan and the launches of sk_dtw_pairs (sk_pairs.hip): d_values / d_out on the device, off / pairs on the host;
// sequence s is d_values[off[s] - off0 .. off[s + 1] - off0).  sk_pairs_check: the argument checks alone (nothing launched)
int sk_pairs_check(const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs, int32_t mode, const void *out);
int sk_pairs_run(sk_ctx *c, const double *d_values, const int64_t *off, int64_t off0, int32_t nseq, const sk_pair *pairs,
                 int64_t npairs, int32_t mode, sk_hit *d_out);
// the warping paths of a pair list (sk_pairpath.hip): the checks of sk_pairs_check, then (have_records == 0) sk_pairs_run
// into d_rec, then the spans of every pair into d_spans [sum N][2], pair after pair in list order.  d_values / d_rec /
// d_spans on the device.  Resets the mismatch counter (sk_path_begin) and synchronises between its two launches.
int sk_pair_paths_run(sk_ctx *c, const double *d_values, const int64_t *off, int64_t off0, int32_t nseq, const sk_pair *pairs,
                      int64_t npairs, int32_t mode, sk_hit *d_rec, int32_t have_records, int32_t *d_spans);
// the exact single pass that also stores every read's last row (cost, back-trace start) at r * max_len (sk_sdtw.hip)
int sk_launch_sdtw_rows(sk_ctx *c, const sk_sdtw_args *a, double *rowD, int32_t *rowS);
// hit lists (sk_hits.hip): up to K disjoint matches per read from those rows; out [nreads][K], count [nreads]
int sk_launch_hits_select(sk_ctx *c, const double *rowD, const int32_t *rowS, int64_t row_stride, const sk_hit *rec,
                          int32_t nreads, int32_t K, double max_dist, sk_hit *out, int32_t *count);
// hit lists over a table of ragged rows (sk_pairhits.hip): tab[0 .. nrows) on the host (reordered: longest first) is
// copied to entry `at` of c->rowhit (sk_rowhits_reserve: room for that many entries) and selected from -- rows of up to
// 4 096 columns by one wavefront each, longer ones by a workgroup each; *long_rows += the latter
int sk_rowhits_reserve(sk_ctx *c, int64_t nrows);
int sk_launch_rowhits(sk_ctx *c, sk_rowhit_entry *tab, int64_t at, int32_t nrows, const double *rowD, const int32_t *rowS,
                      int32_t K, double max_dist, sk_hit *out, int32_t *count, int64_t *long_rows);
// the plan and the launches of sk_dtw_pairs_hits (sk_pairs.hip): d_values / d_out [npairs][K] / d_count on the device,
// off / pairs on the host; checked by the caller (sk_pairs_check, the hit-list rules), npairs > 0
int sk_pairs_hits_run(sk_ctx *c, const double *d_values, const int64_t *off, int64_t off0, int32_t nseq, const sk_pair *pairs,
                      int64_t npairs, int32_t K, double max_dist, sk_hit *d_out, int32_t *d_count);
// read background (sk_bg.hip): mean, std, median, MAD and the count below mean - std of each read's last row, in numpy's
// order and bit for bit; rec supplies n and the flags (flagged reads: NaN fields, below -1); out [nreads]
int sk_launch_row_background(sk_ctx *c, const double *rowD, int64_t row_stride, const sk_hit *rec, int32_t nreads,
                             sk_bg_rec *out);
// alignment paths (sk_path.hip): spans [nreads][K][nmotif][2] of the hits [nreads][K] of prepared reads (samples / prep /
// stride / off / max_len as sk_sdtw_args); d_motif: the motif on the DEVICE.  sk_path_begin: once per API call, before
// the first launch (zeroes the call's mismatch counter).
struct sk_path_args {
    int            feed;
    const void    *samples;
    const void    *samples_raw = nullptr;
    int64_t        stride = 0;
    const int64_t *off = nullptr;
    const sk_prep *prep = nullptr;
    int32_t        nreads = 0;
    int64_t        max_len = 0;
    const double  *d_motif = nullptr;
    int32_t        nmotif = 0;
    const sk_hit  *hits = nullptr;
    int32_t        K = 1;
    int32_t       *spans = nullptr;
};
int sk_path_begin(sk_ctx *c);
int sk_launch_paths(sk_ctx *c, const sk_path_args *p);
// events (sk_events.hip): one sk_event per motif point of the hits whose spans sk_launch_paths left in p->spans (same
// arguments); events [nreads][K][nmotif].  A hit with spans -1 gets NaN / -1 / 0 records.
int sk_launch_events(sk_ctx *c, const sk_path_args *p, sk_event *events);
// pooling: d_ev [nhits][N] and d_use [nhits] (or nullptr) -> d_out [N]; d_idx (nhits ints) and d_cnt (one int): scratch
int sk_launch_events_pool(sk_ctx *c, const sk_event *d_ev, const uint8_t *d_use, int64_t nhits, int32_t N,
                          int32_t *d_idx, int32_t *d_cnt, sk_pool_rec *d_out);
// fixed-point screening + certified window over all reads (sk_sdtwq.hip); leaves the retry list on the device
int sk_launch_sdtw_screen(sk_ctx *c, const sk_sdtw_args *a, int ck, int span, int span2,
                          int32_t *d_retry_cnt, int32_t *d_retry, int32_t *d_early_cnt, int32_t *d_early);

// ---- adaptive-band DTW over a pair list (sk_band.hip) ----
// sk_band_check: the argument checks alone (host only, nothing launched; usable before a context exists).
// sk_band_run: the checks, the plan and the one launch; d_values / d_rec / d_spans on the device (d_spans == nullptr:
// records only), off / pairs on the host, sequence s = d_values[off[s] - off0 .. off[s + 1] - off0).  With spans it
// resets the mismatch counter (sk_path_begin).
int sk_band_check(const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs, int32_t band, int32_t end_mode,
                  const void *out);
int sk_band_run(sk_ctx *c, const double *d_values, const int64_t *off, int64_t off0, int32_t nseq, const sk_pair *pairs,
                int64_t npairs, int32_t band, int32_t end_mode, sk_hit *d_rec, int32_t *d_spans);

// ---- motif panel inside a search region (sk_panel.hip) ----
// slice(begin, end).indices(len) of a Python slice with step 1: *lo = start, *hi = stop (stop < start: empty).
// clamped (optional): bit 0 / bit 1 = begin / end lay outside the read and was cut to it.
__host__ __device__ static inline void sk_slice_indices(int32_t len, int32_t begin, int32_t end, int32_t *lo, int32_t *hi, int *clamped = nullptr)
{
    int64_t s = begin, e = end;
    int cl = 0;
    if (s < 0) { s += len; if (s < 0) { s = 0; cl |= 1; } } else if (s > len) { s = len; cl |= 1; }
    if (e < 0) { e += len; if (e < 0) { e = 0; cl |= 2; } } else if (e > len) { e = len; cl |= 2; }
    *lo = (int32_t)s; *hi = (int32_t)e;
    if (clamped) *clamped = cl;
}
// k_region_rows: read r's slice [begin:end] (or d_win[r][0] : d_win[r][1]) of its first min(d_len[r], stride) samples ->
// d_rows + r * wstride (zero padded to wstride, a multiple of 8; a slice longer than wstride is cut to it), its length
// -> d_wlen[r], the resolved raw begin -> d_from[r] (may be nullptr).
int sk_launch_region_rows_i16(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              int32_t begin, int32_t end, const int32_t *d_win, int16_t *d_rows, int64_t wstride,
                              int32_t *d_wlen, int32_t *d_from);
// float64 reads: window r = d_sig[d_src[r] .. d_src[r] + (d_woff[r + 1] - d_woff[r])) -> d_out + d_woff[r]
int sk_launch_region_rows_f64(sk_ctx *c, const double *d_sig, const int64_t *d_src, const int64_t *d_woff, int32_t nreads,
                              double *d_out);
// Lays the motifs of a call out per lane, groups them by (L, R) and uploads layouts, table, mean and sd (c->panel);
// `pairs`: reads x motifs the call will sweep at a time (chooses four reads or one read per wavefront).
int sk_panel_plan(sk_ctx *c, const double *motifs, const int32_t *motif_off, int32_t nmotifs, const double *mean,
                  const double *sd, int64_t pairs);
// The exact sweep over prepared reads (feed / samples / samples_raw / stride / off / prep / nreads / max_len of `base`) and
// every motif of the plan: motif k's record of read r -> d_all[k * out_stride + r].  motifs: the caller's (host), for
// the chained launcher of the long ones.
int sk_launch_panel_dtw(sk_ctx *c, const sk_sdtw_args *base, const double *motifs, const int32_t *motif_off,
                        sk_hit *d_all, int64_t out_stride);
// k_panel_rank: scores and ranking of nreads reads from d_all[k * out_stride + r] -> d_out[r]
int sk_launch_panel_rank(sk_ctx *c, const sk_hit *d_all, int64_t out_stride, int32_t nreads, int32_t nmotifs,
                         sk_panel_rec *d_out);

// ---- dRNA --signal branch (rolling mean): statistics + masks (sk_prep.hip), scan (sk_drna_walk.hip) ----
struct sk_roll_params;
// comp / prep as left by sk_launch_prep_i16; psum: nreads * (stride + 1) int64 scratch; masks: two
// transposed bit masks (t < bot, t > bot), `words` words per read each, word wi of read r at [wi * nreads + r]
bool sk_roll_stream_ok(int64_t stride, int32_t w, int32_t lo, int32_t hi);   // can the streaming kernel take these rows?
int sk_launch_roll_stream(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, int32_t lo,
                          int32_t hi, int32_t w, double std_scale, sk_prep *d_prep, uint64_t *d_below, uint64_t *d_above,
                          int32_t *d_redo /* [nreads + 2] */);
size_t sk_roll_one_lds(int64_t stride, int32_t w);      // LDS of the one-look kernel for these rows (0: they do not fit)
int sk_launch_roll_one(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, int32_t lo,
                       int32_t hi, int32_t w, double std_scale, sk_prep *d_prep, uint64_t *d_below, uint64_t *d_above);
int sk_launch_roll_stats(sk_ctx *c, const int16_t *d_comp, int64_t stride, sk_prep *d_prep, int32_t nreads,
                         int32_t w, double std_scale, int64_t *d_psum, uint64_t *d_below, uint64_t *d_above);
int sk_launch_roll_walk(sk_ctx *c, const uint64_t *d_below, const uint64_t *d_above, const sk_prep *d_prep,
                        int32_t nreads, const sk_roll_params *p, int32_t *d_xy, int32_t *d_found, int64_t row_words = 0);

// ---- segmenter, streaming path (sk_segstat.hip) ----
int  sk_segment_fast_row16(int64_t stride);
bool sk_segment_fast_applies(const void *d_sig, int64_t stride, int32_t lo, int32_t hi, double std_scale);
// d_cal != nullptr: the pA route in the raw domain (round 6) -- [nreads][2] = {offset, range / digitisation}; lo / hi are
// then the limits in pA and d_scratch holds num_cu rows of `stride` doubles for the numpy-order redo
int  sk_launch_segment_fast(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                            const sk_seg_params *p, int32_t lo, int32_t hi, sk_prep *d_prep, void *d_mask2,
                            int32_t *d_retry, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs,
                            const double *d_cal = nullptr, double *d_scratch = nullptr);
bool sk_segment_pa_applies(const void *d_sig, int64_t stride, double std_scale);
int  sk_launch_prep_pa_listed(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, const double *d_cal,
                              const int32_t *d_list, const int32_t *d_count, int grid, double lo, double hi, double std_scale,
                              double *d_scratch, int64_t scratch_stride, sk_prep *d_prep, void *d_mask2, int row16);

// the statistics and the redo of sk_launch_segment_fast without its walk (int16 route; d_retry: nreads + 16 ints)
int  sk_launch_segment_masks(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                             double std_scale, int32_t lo, int32_t hi, sk_prep *d_prep, void *d_mask2, int32_t *d_retry);

// ---- segmenter parameter sweep (sk_sweep.hip) ----
// One set of a sweep as the walk holds it (a lane's parameters); `index`: its place in the caller's list.
struct sk_sweep_lane {
    int32_t error, corrector, window, seg_dist, first_len, stall_start, gap_dist, index;
};
// The sets that share one mask pass -- equal (lim_low, lim_hi, std_scale) bit patterns -- as runs of `lanes`: nfast sets
// that take the run-hopping walk from `first`, then ngen that take the per-sample one.  `rep`: one of its sets.
struct sk_sweep_group {
    int32_t rep, first, nfast, ngen;
};
// Groups the sets (in the order of their first member) and lays out their lanes; the lanes go to the device as they are.
void sk_sweep_plan(const sk_seg_sweep_set *sets, int32_t nsets, std::vector<sk_sweep_group> &groups,
                   std::vector<sk_sweep_lane> &lanes);
// The walk of `nlanes` sets of one kind (fast: the run-hopping form) over the entries of nreads reads (row16 per read, read r
// clamped to min(d_len[r], mmax) samples); adds into d_sums[lane.index]; d_recs != nullptr: record of (set, read r) at
// d_recs[lane.index * rec_stride + r].
int  sk_launch_seg_sweep_walk(sk_ctx *c, const void *d_mask2, int row16, const int32_t *d_len, int64_t mmax, int32_t nreads,
                              const sk_sweep_lane *d_lanes, int32_t nlanes, bool fast, sk_seg_sweep_sum *d_sums,
                              sk_seg_sweep_rec *d_recs, int64_t rec_stride);

// ---- dRNA slow5-branch walk (sk_drna_walk.hip) ----
struct sk_drna_params;
int sk_launch_drna_walk(sk_ctx *c, const uint64_t *d_mask, int64_t mask_rows, const sk_prep *d_prep,
                        int32_t nreads, const sk_drna_params *p, int32_t *d_segs, int32_t *d_nsegs,
                        int32_t max_segs);

// ---- synth (sk_synth.hip) ----
int sk_launch_synth(sk_ctx *c, int16_t *d_sig, int64_t stride, int32_t nreads, int32_t nsamples,
                    uint64_t seed, const int16_t *d_motif_i16, int32_t nmotif, int64_t row0 = 0,
                    int hit_pm = 500, int stretch_pm = 0, int stretch = 1);
int sk_launch_synth_windows(sk_ctx *c, int16_t *d_sig, int64_t stride, int32_t nreads, int32_t nsamples,
                            uint64_t seed, int64_t row0, const int16_t *d_tmpl, int32_t ntmpl, float sigma);
int sk_launch_raw_to_pa(sk_ctx *c, const int16_t *d_sig, int64_t stride, int32_t nreads, int32_t nsamples,
                        double offset, double raw_unit, double *d_out, int64_t *d_off);
int sk_launch_centi_to_f64(sk_ctx *c, const int32_t *d_centi, int64_t total, double *d_out);
// ragged form with per-read constants: read r's len = off[r+1] - off[r] samples, cal[2r] = offset, cal[2r+1] = raw unit
int sk_launch_rows_to_pa(sk_ctx *c, const int16_t *d_sig, int64_t stride, int32_t nreads, const int64_t *d_off,
                         const double *d_cal, double *d_out);

// ---- float64 reads, streaming statistics (sk_f64stat.hip) + the numpy-order redo of its uncertified reads ----
bool sk_f64_fast_applies(int64_t maxlen, double std_scale);
int  sk_f64_row16(int64_t maxlen);
int  sk_launch_f64_stats(sk_ctx *c, const double *d_sig, const int64_t *d_off, const int32_t *d_rlen, int32_t nreads, int64_t maxlen,
                         double lo, double hi, int mode, double std_scale, sk_prep *d_prep, void *d_mask2, int row16,
                         int32_t *d_len, int32_t *d_retry, double *d_comp);
int  sk_launch_prep_f64_listed(sk_ctx *c, const double *d_sig, const int64_t *d_off, const int32_t *d_list,
                               const int32_t *d_count, int grid, double lo, double hi, int mode, double std_scale,
                               double *d_comp_or_scratch, int64_t scratch_stride, sk_prep *d_prep, void *d_mask2,
                               int row16, const int32_t *d_rlen = nullptr);
int  sk_launch_seg_walk_masks(sk_ctx *c, const void *d_mask2, int row16, const int32_t *d_len, int32_t nreads,
                              const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs);

// ---- segment levels (sk_seglev.hip) ----
// Per-segment and per-read signal statistics over the {in band, kept} entries a segmenter route left at d_mask2 (row16 per
// read; read r has min(d_len[r], mmax) raw samples) and the segments its walk reported (d_segs [nreads][max_segs][2],
// d_nsegs [nreads]).  feed: SK_FEED_I16 (samples = int16 rows of `stride`) or SK_FEED_F64_NORM (samples = float64, read
// r at d_off[r]).  levels [nreads][max_segs], read_level [nreads].  d_work: sk_seglev_work_bytes(..) bytes of scratch.
size_t sk_seglev_work_bytes(sk_ctx *c, int32_t nreads, int32_t max_segs, int64_t mmax);
int sk_launch_seg_levels(sk_ctx *c, int feed, const void *samples, int64_t stride, const int64_t *d_off,
                         const void *d_mask2, int row16, const int32_t *d_len, int64_t mmax, int32_t nreads,
                         const int32_t *d_segs, const int32_t *d_nsegs, int32_t max_segs, void *d_work,
                         sk_seg_level *levels, sk_seg_level *read_level);

// ---- event detection (sk_detect.hip) ----
// Mark: the mark words of read r (one bit per sample, sk_detect_words(stride) words of 8 bytes per read) at d_words and
// its event count, as int64, at d_cnt[r].  Scan: d_off[0 .. nreads) counts -> d_off[0 .. nreads] offsets (d_bsum:
// sk_scan_blocks(nreads) entries).  Fill: the records at d_rec[d_off[r] ..], nothing when d_off[nreads] > cap.
// sk_detect_work_bytes: the words of nreads rows and the block sums behind them.
int64_t sk_detect_words(int64_t stride);
size_t  sk_detect_work_bytes(int32_t nreads, int64_t stride);
int sk_launch_detect_mark(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                          const sk_det_params *p, void *d_words, int64_t *d_cnt);
int sk_launch_detect_scan(sk_ctx *c, int32_t nreads, int64_t *d_bsum, int64_t *d_off);
int sk_launch_detect_fill(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                          const sk_det_params *p, const void *d_words, const int64_t *d_off, sk_det_event *d_rec, int64_t cap);

// ---- signal HMM (sk_hmm.hip) ----
// the pA value of a raw sample under a read's {offset, unit} pair (sk_pa_calib): one add, one multiply -- what
// SquigglePull's text rounds to two decimals and what the HMM's emissions take unrounded
__host__ __device__ static inline double sk_raw_to_pa(double raw, double offset, double unit)
{
    const double x = raw + offset;
    return x * unit;
}
// nullptr when the model keeps the rules of the header's "signal HMM" section, else what it breaks
const char *sk_hmm_model_error(const sk_hmm_model *m);
// Viterbi records of nreads reads -> d_rec[0 .. nreads): int16 rows (d_cal: {offset, unit} per read, or nullptr), or
// ragged float64 values (read r = d_values[d_off[r] .. d_off[r + 1])).  limit > 0: the first min(len, limit) samples.
int sk_launch_hmm_i16(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                      const double *d_cal, const sk_hmm_model *m, int32_t limit, sk_hmm_rec *d_rec);
int sk_launch_hmm_f64(sk_ctx *c, const double *d_values, const int64_t *d_off, int32_t nreads, const sk_hmm_model *m,
                      int32_t limit, sk_hmm_rec *d_rec);
// State paths (the header's "signal HMM: state paths").  npad: the most samples a read of the call can use (maxlen: the
// stride, or the longest ragged read); the back pointers of a slice of whole 64-read groups, its counts and the scan's
// block sums take sk_hmm_path_work_bytes(nreads, npad) bytes -- never more than the budget (16 GiB, or
// SK_HMM_SCRATCH_MB) unless one group alone needs more.  Paths: records, offsets (continuing from d_off[0] unless
// `first`) and state / start / length of every segment, slice by slice; stats: n1, sum, sumsq of the whole call.  Reads
// whose segments end past cap get no records.
int64_t sk_hmm_npad(int64_t maxlen, int32_t limit);
int64_t sk_hmm_slice_groups(int32_t nreads, int64_t npad);
size_t  sk_hmm_path_work_bytes(int32_t nreads, int64_t npad);
int sk_launch_hmm_paths(sk_ctx *c, int feed, const void *d_sig, int64_t stride, const int32_t *d_len, const int64_t *d_roff,
                        int32_t nreads, const double *d_cal, const sk_hmm_model *m, int32_t limit, int64_t npad, void *d_work,
                        int first, sk_hmm_rec *d_rec, int64_t *d_off, sk_hmm_seg *d_seg, int64_t cap);
int sk_launch_hmm_stats(sk_ctx *c, int feed, const void *d_sig, int64_t stride, const int64_t *d_roff, int32_t nreads,
                        const double *d_cal, const sk_hmm_model *m, const int64_t *d_off, void *d_seg, int64_t cap);

// ---- signal HMM posteriors (sk_hmm_post.hip) ----
// Forward-backward per read (the header's "signal HMM: posteriors"): records -> d_post, soft counts -> d_counts (or
// nullptr), dense rows -> d_gamma + d_goff[r] * 6 (or both nullptr).  npad as for the state paths; the scratch of a slice
// of whole 64-read groups takes sk_hmm_post_work_bytes(nreads, npad) bytes, within the state paths' budget.
size_t sk_hmm_post_work_bytes(int32_t nreads, int64_t npad);
int sk_launch_hmm_post(sk_ctx *c, int feed, const void *d_sig, int64_t stride, const int32_t *d_len, const int64_t *d_roff,
                       int32_t nreads, const double *d_cal, const sk_hmm_model *m, int32_t limit, int64_t npad, void *d_work,
                       sk_hmm_post *d_post, sk_hmm_counts *d_counts, const int64_t *d_goff, double *d_gamma);

// ---- MotifSeq sessions (sk_stream.hip) ----
// The session behind the entry points of sk_api.hip: arguments checked there, every pointer a device pointer here.
// open: motifs / motif_off on the host, limits already clamped.  push: one ingest, statistics of the slots whose
// calibration ends in this call, one sweep per motif, the records to d_out [nmotifs][m]; rows == nullptr: no samples
// (flush != 0: the named slots end their calibration).  reset: d_center / d_scale both nullptr or both [m].
int sk_stream_session_open(sk_ctx *c, const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                           const sk_stream_params *p, int32_t *handle);
int sk_stream_session_info(sk_ctx *c, int32_t handle, int32_t *nslots, int32_t *nmotifs);   // SK_ERR_INVALID: unknown handle
int sk_stream_session_push(sk_ctx *c, int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows,
                           int64_t stride, const int32_t *d_len, int flush, sk_stream_rec *d_out);
int sk_stream_session_reset(sk_ctx *c, int32_t handle, const int32_t *d_slots, int32_t m, const double *d_center,
                            const double *d_scale);
// the session's staging room for the host entry points: `bytes` of device memory that lives until the next call
int sk_stream_session_stage(sk_ctx *c, int32_t handle, int which, size_t bytes, void **p);
int sk_stream_session_close(sk_ctx *c, int32_t handle);
void sk_stream_close_all(sk_ctx *c);        // sk_shutdown: the context's device is current

// ---- mapping sessions (sk_mapstream.hip) ----
// The session behind sk_map_*: arguments that need no session are checked in sk_api.hip, the rest (handle, slots against
// nslots) here.  open: targets / target_off on the host.  push: slots and off on the host, d_values (chunk i at
// off[i] - off[0]) and d_out [ntargets][m] on the device; nothing is synchronised behind the launches.
int sk_map_session_open(sk_ctx *c, const double *targets, const int64_t *target_off, int32_t ntargets, int32_t nslots,
                        int32_t *handle);
int sk_map_session_info(sk_ctx *c, int32_t handle, int32_t *nslots, int32_t *ntargets);      // SK_ERR_INVALID: unknown handle
int sk_map_session_check_slots(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m);
int sk_map_session_push(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, const double *d_values,
                        const int64_t *off, sk_map_rec *d_out);
int sk_map_session_reset(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m);
// hit lists from the stored rows of the named slots (checked against nslots here), every target: d_out [ntargets][m][K],
// d_count [ntargets][m] on the device; nothing is swept, nothing of the session changes
int sk_map_session_hits(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, int32_t K, double max_dist, sk_hit *d_out,
                        int32_t *d_count);
int sk_map_session_stage(sk_ctx *c, int32_t handle, int which, size_t bytes, void **p);
int sk_map_session_close(sk_ctx *c, int32_t handle);
void sk_map_close_all(sk_ctx *c);           // sk_shutdown: the context's device is current

// ---- SquigglePull text (sk_pull.hip) ----
// ---- event sessions (sk_evstream.hip) ----
// The session behind sk_evs_*: arguments that need no session are checked in sk_api.hip, the rest (handle, slots against
// nslots, ended slots, the 2^31 - 1 samples of a slot) here.  A push leaves its staging rows and offsets in the session;
// sk_evs_session_gather compacts them to a device buffer, as often as asked, until the next push.
int64_t sk_evs_session_rows(sk_ctx *c, int32_t handle, int64_t maxlen);   // staging rows per entry of such a push
int sk_evs_session_open(sk_ctx *c, const sk_det_params *p, int32_t nslots, int32_t *handle);
int sk_evs_session_info(sk_ctx *c, int32_t handle, int32_t *nslots);                         // SK_ERR_INVALID: unknown handle
int sk_evs_session_check(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, const int32_t *len);
int sk_evs_session_check_cap(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, const int32_t *len, int64_t cap);
int sk_evs_session_stage(sk_ctx *c, int32_t handle, int which, size_t bytes, void **p);
int sk_evs_session_push(sk_ctx *c, int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows, int64_t stride,
                        const int32_t *d_len, const int32_t *d_end, int64_t per, int64_t *d_off, const int32_t *host_slots,
                        const int32_t *host_len, const int32_t *host_end);
int sk_evs_session_gather(sk_ctx *c, int32_t handle, sk_det_event *d_rec, int64_t cap);
int sk_evs_session_last(sk_ctx *c, int32_t handle, const int64_t **d_off, int32_t *m);
int sk_evs_session_staging(sk_ctx *c, int32_t handle, const sk_det_event **d_stage, int64_t *per);
int sk_evs_session_reset(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m);
int sk_evs_session_close(sk_ctx *c, int32_t handle);
void sk_evs_close_all(sk_ctx *c);           // sk_shutdown: the context's device is current

// ---- HMM sessions (sk_hmmstream.hip) ----
// The kernel, the session and the sk_hmms_* entries are all in that file; the runtime only closes what is left open.
// sk_hmms_session_*: the session without the entry checks, for a gated live session's own HMM session -- device
// pointers, nothing synchronised, k_hmms_push and k_hmms_reset as the entries launch them.
#define SK_HMMS_CAP 0x7fffff00              // samples a slot can hold
void sk_hmms_close_all(sk_ctx *c);          // sk_shutdown: the context's device is current
int sk_hmms_session_open(sk_ctx *c, const sk_hmm_model *model, int32_t nslots, int32_t *handle);
int sk_hmms_session_push_dev_i16(sk_ctx *c, int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows,
                                 int64_t stride, const int32_t *d_len, sk_hmms_rec *d_out);
int sk_hmms_session_reset_dev(sk_ctx *c, int32_t handle, const int32_t *d_slots, int32_t m, const double *d_cal2);
int64_t sk_hmms_session_bytes(sk_ctx *c, int32_t handle);
int sk_hmms_session_close(sk_ctx *c, int32_t handle);

// ---- live mapping sessions (sk_live.hip) ----
// The session behind sk_live_*: an event session and a mapping session of its own (opened and closed through the
// functions above: one handle of each table while it is open), the bridge between them and the decision summary.
// Arguments that need no session are checked in sk_api.hip.  push: host_slots checked by the caller's entry against
// nothing but the ABI's limits -- the session checks them against nslots; every d_ pointer a device pointer; host_len /
// host_end as in sk_evs_session_push (nullptr: a device-form push).  d_best is written only when rule is given.
int sk_live_session_open(sk_ctx *c, const sk_det_params *p, int32_t calib, const double *targets, const int64_t *target_off,
                         int32_t ntargets, int32_t nslots, const sk_hmm_model *model /* nullptr: ungated */,
                         const sk_live_gate *gate, int32_t *handle);
int sk_live_session_info(sk_ctx *c, int32_t handle, int32_t *nslots, int32_t *ntargets, int32_t *evs, int32_t *map);
// the last push's gate records and HMM records (device, [m]); SK_ERR_INVALID on an ungated session
int sk_live_session_gate_last(sk_ctx *c, int32_t handle, const sk_live_gate_info **d_gate, const sk_hmms_rec **d_rec, int32_t *m);
int sk_live_session_check(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, int64_t stride, const int32_t *len);
int sk_live_session_stage(sk_ctx *c, int32_t handle, int which, size_t bytes, void **p);
int sk_live_session_push(sk_ctx *c, int32_t handle, const int32_t *host_slots, const int32_t *d_slots, int32_t m,
                         const int16_t *d_rows, int64_t stride, const int32_t *d_len, const int32_t *d_end, int64_t per,
                         const int32_t *host_len, const int32_t *host_end, const sk_live_rule *rule, sk_map_rec *d_out,
                         sk_live_info *d_info, sk_live_best *d_best);
int sk_live_session_last(sk_ctx *c, int32_t handle, const int64_t **d_off, const double **d_values, int32_t *m);
int sk_live_session_best_ms(sk_ctx *c, int32_t handle, float *ms);
int sk_live_session_gate_ms(sk_ctx *c, int32_t handle, float *hmm_ms, float *gate_ms);
int sk_live_session_reset(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, const double *cal2 /* gated only */);
int sk_live_session_close(sk_ctx *c, int32_t handle);
void sk_live_close_all(sk_ctx *c);          // sk_shutdown, BEFORE the tables it holds handles of are emptied

// ---- the gate of a gated live session (sk_livegate.hip) ----
// The kernels between the inner sessions of a gated live session: the HMM chunk lengths ahead of the HMM push, and
// k_live_gate behind both pushes -- decision, hold ring, released rows.  Every pointer a device pointer.
struct sk_gate_slot {                       // 40 bytes: a slot's gate record and what the ring remembers
    sk_live_gate_info g;
    int32_t last_drop;                      // the start of the event the ring overwrote last (dropped > 0)
    int32_t pad;
};
struct sk_gate_args {
    sk_gate_slot        *state;             // [nslots]
    sk_det_event        *ring;              // [nslots][G]: event number e of the slot at e % G
    const sk_live_info  *live;              // [nslots]: the live side's records (ended, as of the push before)
    int32_t              nslots, G;
    const int32_t       *slots;             // [m]
    int32_t              m;
    const int32_t       *len, *end;         // [m]; end may be nullptr
    const sk_hmms_rec   *hrec;              // [m]: the HMM push's records
    const sk_det_event  *stage;             // [m][per]: the event push's staging rows
    int64_t              per;
    const int64_t       *eoff;              // [m + 1]: the event push's offsets
    sk_det_event        *rel;               // [m][G + per] out: the released rows
    int64_t             *rcnt;              // [m] out: their counts
    sk_live_gate_info   *ginfo;             // [m] out
    sk_live_gate         rule;
};
int sk_livegate_reset(sk_ctx *c, sk_gate_slot *state, int32_t nslots, const int32_t *d_slots, int32_t m);
int sk_livegate_lengths(sk_ctx *c, const sk_gate_args &a, int32_t *d_hlen);
int sk_livegate_release(sk_ctx *c, const sk_gate_args &a);

// ---- reference pile-up (sk_pileup.hip) ----
// The header's "Reference pile-up": every array on the device but tlen (host).  d_use / d_dwell / d_target / d_shift may
// be nullptr (all used / ones / zeros / zeros); d_ent_off and d_ent_row both nullptr or both set.  Nothing is written to
// d_out / d_ent_off / d_ent_row before the checks have passed (one read-back of the counters).
int sk_pileup_run(sk_ctx *c, const int64_t *d_span_off, const int32_t *d_spans, const double *d_value, const int32_t *d_dwell,
                  const int32_t *d_target, const int32_t *d_shift, const uint8_t *d_use, int32_t npairs, int64_t nrows,
                  const int64_t *tlen, int32_t ntargets, sk_pile_rec *d_out, int64_t *d_ent_off, int32_t *d_ent_row,
                  int64_t ent_cap);

// exclusive int64 scan: out[0 .. n] = prefix sums of v[0 .. n) (out may be v); bsum: sk_scan_blocks(n) entries
int64_t sk_scan_blocks(int64_t n);
int     sk_launch_scan_i64(sk_ctx *c, const int64_t *v, int64_t n, int64_t *bsum, int64_t *out);
int64_t sk_pull_tile_cap(int32_t nreads, int64_t stride);   // tiles the rows can hold at most
// d_cal: {offset, raw unit} per read, nullptr in raw mode.  Count: tile0 (nreads + 1), tb (tile_cap + 1) and
// line_off (nreads + 1) get their exclusive scans, *d_err |= 1 for a value the formatter cannot print.
int sk_launch_pull_count(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                         const double *d_cal, const int64_t *d_poff, int64_t *d_tile0, int64_t *d_tb, int64_t tile_cap,
                         int64_t *d_bsum, int64_t *d_line_off, int32_t *d_err);
int sk_launch_pull_write(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                         const double *d_cal, const char *d_prefix, const int64_t *d_poff, const int64_t *d_tile0,
                         const int64_t *d_tb, int64_t tile_cap, const int64_t *d_line_off, char *d_out);
