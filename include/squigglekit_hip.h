/*
 * squigglekit_hip.h -- C ABI of libsquigglekit_hip.so (MI355X / gfx950).
 *
 * The reference (Psy-Fer/SquiggleKit) has no FFI: its hot path sits behind two
 * in-process Python call boundaries,
 *     segmenter.get_segs(sig, args)          /root/reference/segmenter.py:399
 *     mlpy.dtw_subsequence(model, sig)       /root/reference/MotifSeq.py:437
 * wrapped by per-read loops (segmenter.py:189-230, MotifSeq.py:261-298) that
 * filter (scale_outliers) and normalise each read first.  This header is what
 * a ctypes binding at those two call sites binds instead (INTEGRATION.md shows
 * the stub).  Batch entry points take many reads per call because one read is
 * far too little work for a GPU; the single-pair entry points keep the
 * reference's one-call-per-read shape.
 *
 * Conventions
 *   - plain pointers and sizes only; caller owns every buffer; the library
 *     keeps no caller pointer after a call returns.
 *   - every function returns SK_OK (0) or a negative sk_status; the message is
 *     available from sk_last_error() (thread local).
 *   - "host" entry points take host pointers and do H2D / kernels / D2H;
 *     "_dev" entry points take device pointers obtained from sk_dev_alloc()
 *     and leave results in HBM (what bench.py times).
 *   - no CPU fallback exists: without a usable HIP device every compute entry
 *     point fails with SK_ERR_NO_DEVICE.
 */
#ifndef SQUIGGLEKIT_HIP_H
#define SQUIGGLEKIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sk_status {
    SK_OK              =  0,
    SK_ERR_INVALID     = -1,   /* bad argument (NULL, negative size, bad params)        */
    SK_ERR_NO_DEVICE   = -2,   /* no HIP device / sk_init not called / device lost      */
    SK_ERR_HIP         = -3,   /* a HIP runtime call failed (message has the detail)    */
    SK_ERR_NOMEM       = -4,   /* device or host allocation failed                      */
    SK_ERR_UNSUPPORTED = -5,   /* shape outside what the kernels cover (message says)   */
    SK_ERR_OVERFLOW    = -6    /* max_segs too small for at least one read              */
} sk_status;

/* scale modes of MotifSeq.py -l/--scale (MotifSeq.py:96) */
enum { SK_SCALE_MEDMAD = 0, SK_SCALE_ZSCALE = 1 };

/* flags in sk_hit.flags */
enum {
    SK_FLAG_EMPTY      = 1,    /* no sample survived scale_outliers: dist = NaN, start=end=-1 */
    SK_FLAG_DEGENERATE = 2,    /* medmad with MAD == 0 (reference divides by zero)            */
    SK_FLAG_RECENTRE   = 4     /* float64 zscale: sklearn.preprocessing.scale subtracted the residual mean a
                                  second time ("mean not close to zero", near-constant or huge-valued
                                  data, MotifSeq.py:187-191); applied here too -- informational        */
};

/* get_segs parameters: the argparse flags of segmenter.py:65-96 that reach
 * scale_outliers (segmenter.py:311-318) and get_segs (segmenter.py:399-470). */
typedef struct sk_seg_params {
    int32_t error;       /* -e/--error      default 5    */
    int32_t corrector;   /* -c/--corrector  default 50   */
    int32_t window;      /* -w/--window     default 150  */
    int32_t seg_dist;    /* -d/--seg_dist   default 50   */
    double  std_scale;   /* -t/--std_scale  default 0.75 */
    double  stall_len;   /* -l/--stall_len  default 0.25 */
    int32_t lim_low;     /* -lim_low        default 0    */
    int32_t lim_hi;      /* -lim_hi         default 900  */
} sk_seg_params;

/* One MotifSeq hit: what get_region_multi (MotifSeq.py:431-449) derives from
 * dist, path[1][0], path[1][-1].  24 bytes. */
typedef struct sk_hit {
    double  dist;        /* cost[-1, argmin]                                   */
    int32_t start;       /* path[1][0]   (index into the FILTERED signal)      */
    int32_t end;         /* path[1][-1]  (argmin of the last row)              */
    int32_t n;           /* samples that survived scale_outliers               */
    int32_t flags;       /* SK_FLAG_*                                          */
} sk_hit;

/* ---- runtime --------------------------------------------------------- */
const char *sk_version(void);
const char *sk_last_error(void);
int  sk_device_count(void);                 /* >= 0, or negative sk_status                */
int  sk_init(int device);                   /* bind the calling thread to `device`        */
/* The same with an explicit context slot (0..15; sk_init uses slot == device).  Every slot has its own stream and
 * scratch, so several host threads (or ranks) can share one GPU: how the sharded multi-GPU paths are exercised on
 * a one-GPU box.  The RCCL entry points still need one device per rank. */
int  sk_init_slot(int slot, int device);
int  sk_shutdown(void);                     /* free every per-device context              */
int  sk_sync(void);                         /* wait for the bound device's stream         */
int  sk_device_name(char *buf, int cap);    /* marketing/gcn name of the bound device     */
/* "0000:c1:00.0" of the bound device (cap >= 16): the key of /sys/bus/pci/devices/<id>/local_cpulist -- a multi-GPU
 * host binds each rank's feeder thread to the CPUs next to its GPU (squigglekit_amd/multigpu.py) */
int  sk_device_pci_bus_id(char *buf, int cap);

/* ---- device memory (for *_dev entry points) --------------------------- */
void *sk_dev_alloc(size_t bytes);           /* NULL on failure                            */
int   sk_dev_free(void *dptr);
int   sk_dev_upload(void *dst_dev, const void *src_host, size_t bytes);
int   sk_dev_download(void *dst_host, const void *src_dev, size_t bytes);

/* ---- pinned host memory (optional, for the host entry points) ---------- */
/* The host entry points (sk_*_batch_*) move a large batch in sub-batches, the H2D copy of one under the kernels
 * of the previous one.  With ordinary (pageable) caller memory the copies are staged by the HIP runtime; buffers
 * from sk_host_alloc() are page-locked and go by DMA at PCIe speed.  Either kind may be passed anywhere a host
 * pointer is expected. */
void *sk_host_alloc(size_t bytes);          /* NULL on failure                            */
int   sk_host_free(void *hptr);

/* ---- segmenter path --------------------------------------------------- */
/* Replaces, per read r: scale_outliers(sig) (segmenter.py:209,311-318) then
 * get_segs(sig, args) (segmenter.py:211,399-470).
 *   sig[r*stride .. r*stride+len[r])  raw samples of read r (caller applies
 *                                      the [:Num] cut of segmenter.py:207)
 *   segs[r][k][0..1]                   k-th [start,end] in FILTERED coordinates
 *   nsegs[r]                           number found; 0 == the reference's False
 * Returns SK_ERR_OVERFLOW if some nsegs[r] > max_segs (nsegs is still exact,
 * segs truncated). */
int sk_segment_batch_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                         const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs);
/* float64 samples (pA TSVs; segmenter.py:198-199), ragged: read r is
 * sig[off[r] .. off[r+1]). */
int sk_segment_batch_f64(const double *sig, const int64_t *off, int32_t nreads,
                         const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs);
/* the same with the caller's sig[:Num] cut (segmenter.py:207) applied per read: read r is the first len[r] samples of
 * sig[off[r] .. off[r+1]) (len may be NULL: whole reads) -- a parsed TSV chunk goes in as it is, no repacking. */
int sk_segment_batch_f64_len(const double *sig, const int64_t *off, const int32_t *len, int32_t nreads,
                             const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs);
/* the same for a ragged batch of int32 CENTI-UNITS (sk_tsv_parse_centi: decimal tokens with at most two decimals --
 * SquigglePull's default pA output): sample = centi / 100.0 = float("ddd.dd") bit for bit (segmenter.py:198-199), made
 * on the device; half the bytes over PCIe. */
int sk_segment_batch_centi_len(const int32_t *centi, const int64_t *off, const int32_t *len, int32_t nreads,
                               const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs);
/* raw reads through the pA route -- what segmenter.py does with fast5 / slow5 input unless --raw_signal is given
 * (segmenter.py:345-349, 366-370, 385): np.round((raw + offset) * (float("%.2f" % range) / digitisation), 2), made on
 * the device from the int16 rows, then scale_outliers + get_segs on the float64 values.  calib[3 r ..] = digitisation,
 * offset, range of read r (what a fast5 / BLOW5 record carries).  The caller applies [:Num] via len[]. */
int sk_segment_batch_i16_pa(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const double *calib,
                            const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs);
/* Since round 6 the samples of this route stay int16 on the device: v(x) = rint((x + offset) * unit * 100) / 100 is a
 * non-decreasing function of the sample, so scale_outliers' limits, np.median, np.std (from exact integer centi-pA sums)
 * and the two thresholds of get_segs (segmenter.py:311-318, 410-414, 431) are found in the raw domain -- 2 bytes a sample
 * instead of 8 -- and certified against numpy's rounding; reads that cannot be certified are redone from their float64
 * values in numpy's order.  sk_pa_calib turns the records' {digitisation, offset, range} into the {offset, raw_unit}
 * pairs of the device-resident form (range cut to two decimals first, segmenter.py:385); sk_last_pa_retries: reads of
 * the last such call, all its sub-batches, that took the redo (-1: the call expanded every row to float64 -- rows whose
 * stride is not a multiple of 8 -- or a MotifSeq / segmenter call of another route came after it). */
int sk_pa_calib(const double *calib, int32_t nreads, double *cal2);
int sk_segment_dev_i16_pa(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, const double *d_cal2,
                          const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs);
int sk_last_pa_retries(void);
/* device-resident form of sk_segment_batch_i16 (all pointers device). */
int sk_segment_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                       const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs);
/* device-resident form of sk_segment_batch_f64: d_off holds nreads + 1 ZERO-BASED offsets, total = d_off[nreads]
 * (the library cannot look), max_len >= the longest read. */
int sk_segment_dev_f64(const double *d_sig, const int64_t *d_off, int32_t nreads, int64_t total, int64_t max_len,
                       const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs);

/* ---- segment levels ----------------------------------------------------- */
/* What a segment IS, and where it lies in the raw read.  get_segs returns index pairs into the filtered signal and
 * nothing else (segmenter.py:399-470); a stall, a homopolymer stretch and an adapter differ in level and noise, measured
 * against the read's own median and stdev (the two numbers get_segs builds its band from, segmenter.py:410-414).  With y
 * the read after the [:Num] cut and scale_outliers (segmenter.py:207-209, 311-318) -- the array get_segs is given, int64
 * for integer input, float64 for pA input (segmenter.py:198-201) -- kept[i] the raw index of y[i], and w = y[s:e] for a
 * span [s, e) of y, one record holds, bit for bit what numpy gives on w in its own dtype:
 *   mean   = np.mean(w)                 (np.add.reduce's order, as sk_bg_rec documents it)
 *   std    = np.std(w)                  (ddof 0, two passes, the same order; one sample: 0.0)
 *   median = np.median(w)               (even length: (a + b) / 2 of the two middle values)
 *   mad    = np.median(np.abs(w - median))          (not multiplied by 1.4826)
 *   min, max = float(w.min()), float(w.max())
 *   raw_start = kept[s], raw_end = kept[e - 1] + 1: raw[raw_start:raw_end], filtered, is exactly w
 *   n      = e - s
 * A span with e <= s has six NaNs, raw_start = raw_end = -1 and n = 0; so has every unused slot, and every slot of a
 * read with no surviving sample. */
typedef struct sk_seg_level {       /* 64 bytes */
    double  mean;
    double  std;
    double  median;
    double  mad;
    double  min;
    double  max;
    int32_t raw_start;
    int32_t raw_end;
    int32_t n;
    int32_t pad;                    /* 0 */
} sk_seg_level;
/* levels is [nreads][max_segs]: the record of segs[r][k] = [start, end], end taken as exclusive (the slice
 * segmenter.py's users cut, sig[start:end]).  read_level is [nreads]: the same record over the whole of y, [0, n) --
 * top = median + std * std_scale and bot = median - std * std_scale of segmenter.py:413-414 follow from it in two
 * float64 operations.  segs / nsegs and the return value (SK_ERR_OVERFLOW with the true counts in nsegs included):
 * exactly what the sk_segment_batch_* / sk_segment_dev_* twin returns; the other arguments are its own.  A NULL levels
 * or read_level is SK_ERR_INVALID. */
int sk_segment_levels_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                          const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs,
                          sk_seg_level *levels, sk_seg_level *read_level);
/* ragged float64 reads with the caller's [:Num] cut (sk_segment_batch_f64_len; segmenter.py:198-199, 207) */
int sk_segment_levels_f64_len(const double *sig, const int64_t *off, const int32_t *len, int32_t nreads,
                              const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs,
                              sk_seg_level *levels, sk_seg_level *read_level);
/* the same for int32 centi-units (sk_segment_batch_centi_len) */
int sk_segment_levels_centi_len(const int32_t *centi, const int64_t *off, const int32_t *len, int32_t nreads,
                                const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs,
                                sk_seg_level *levels, sk_seg_level *read_level);
/* device-resident form of sk_segment_levels_i16 (all pointers device but p; nothing is synchronised;
 * segmenter.py:209-211 per read) */
int sk_segment_levels_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs,
                              sk_seg_level *d_levels, sk_seg_level *d_read_level);

/* ---- segmenter parameter sweep ----------------------------------------- */
/* Every set of a grid over the same reads in one call: for set k and read r, what sk_segment_batch_i16 (or the float64
 * route) reports with set k's sk_seg_params, cut to the first two segments, and per set the counts segmenter.py's
 * acceptance tests give (segmenter.py:473-494; -k/-j stall_start, -g/-b gap_dist).  The statistics and masks are built
 * once per distinct (lim_low, lim_hi, std_scale); the walks of all sets that share them read them once.
 * The sets are checked as sk_segment_batch_i16 checks its params (corrector >= 0); SK_ERR_INVALID names the set. */
typedef struct sk_seg_sweep_set {          /* 48 bytes */
    sk_seg_params seg;                     /* the segmenter's flags                  */
    int32_t stall_start;                   /* -j, default 300                        */
    int32_t gap_dist;                      /* -b, default 3000                       */
} sk_seg_sweep_set;

typedef struct sk_seg_sweep_rec {          /* 24 bytes, one per (set, read) */
    int32_t nsegs;                         /* segment count after merges, as sk_segment_batch_i16 reports it */
    int32_t s0_start, s0_end;              /* first segment, filtered coordinates; -1 when nsegs == 0        */
    int32_t s1_start, s1_end;              /* second segment; -1 when nsegs < 2                              */
    int32_t reserved;                      /* 0 */
} sk_seg_sweep_rec;

/* Exact integer counts over the reads, per set.  gap_ok counts a read with exactly ONE segment as passing: the
 * reference's test_segs reads segs[1] inside a bare `except` (segmenter.py:485-492), so such a read is printed. */
typedef struct sk_seg_sweep_sum {          /* 64 bytes */
    int64_t reads;                         /* reads given                                                          */
    int64_t with_segs;                     /* nsegs >= 1: lines segmenter.py prints without -u                     */
    int64_t segs;                          /* sum of nsegs                                                         */
    int64_t stall_ok;                      /* nsegs >= 1 && s0_start <= stall_start: lines with -k -u              */
    int64_t gap_ok;                        /* nsegs >= 1 && (nsegs == 1 || s1_start <= s0_end + gap_dist): -g -u   */
    int64_t stall_gap_ok;                  /* both: lines with -k -g -u                                            */
    int64_t seg0_end_sum;                  /* sum of s0_end over the reads with nsegs >= 1 (filtered coordinates)  */
    int64_t reserved;                      /* 0 */
} sk_seg_sweep_sum;

/* int16 rows as sk_segment_batch_i16 takes them (len[r] in [0, stride]).  sums[nsets]; recs[nsets][nreads] or NULL. */
int sk_segment_sweep_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                         const sk_seg_sweep_set *sets, int32_t nsets, sk_seg_sweep_sum *sums, sk_seg_sweep_rec *recs);
/* the same with every pointer on the device except `sets` (host); sums / recs are device buffers (recs may be NULL). */
int sk_segment_sweep_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                             const sk_seg_sweep_set *sets, int32_t nsets, sk_seg_sweep_sum *d_sums,
                             sk_seg_sweep_rec *d_recs);
/* float64 reads as sk_segment_batch_f64_len takes them: read r is the first len[r] samples of sig[off[r] .. off[r+1])
 * (len may be NULL: whole reads). */
int sk_segment_sweep_f64(const double *sig, const int64_t *off, const int32_t *len, int32_t nreads,
                         const sk_seg_sweep_set *sets, int32_t nsets, sk_seg_sweep_sum *sums, sk_seg_sweep_rec *recs);

/* ---- dRNA adapter segmenter (dRNA_segmenter.py, slow5 branch :85-176) ---- */
/* The script hard-codes these (dRNA_segmenter.py:80-104); they are parameters here. */
typedef struct sk_drna_params {
    int32_t error;          /* 5     tolerated out-of-band samples                         */
    int32_t no_err_thresh;  /* 2500  errors only count from this sample index on           */
    int32_t w;              /* 1200  constant corrector period                             */
    int32_t window;         /* 100   shortest segment kept                                 */
    int32_t seg_dist;       /* 1200  merge distance, and the "adapter found" stop distance */
    int32_t t_start;        /* 1000  statistics come from filtered samples [t_start, t_end) */
    int32_t t_end;          /* 5000                                                        */
    double  std_scale;      /* 0.8   top = median + std * std_scale (one sided: a < top)   */
    int32_t lim_low;        /* 0     scale_outliers limits (dRNA_segmenter.py:329-332)     */
    int32_t lim_hi;         /* 1200                                                        */
} sk_drna_params;
/* Per read: scale_outliers, window statistics, the scan.  segs holds every segment collected
 * before the scan stopped (the script prints the first one only). */
int sk_drna_segment_batch_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                              const sk_drna_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs);

/* ---- dRNA adapter segmenter, --signal branch (dRNA_segmenter.py:272-326): rolling mean -------- */
/* t = pandas.Series(filtered).rolling(window=w).mean(); mn = t.mean(); std = t.std();
 * bot = mn - std * std_scale; runs of t < bot, closed by t > bot, merged when closer than seg_dist;
 * the first segment with lo_thresh <= length <= hi_thresh is reported as (start - shift, end - shift).
 * The script reads `w` before assigning it (:282) -- its commented-out default (:81) is 2000. */
typedef struct sk_roll_params {
    int32_t w;              /* 2000    rolling window (min_periods = w)            */
    int32_t seg_dist;       /* 1500                                                */
    int32_t hi_thresh;      /* 200000                                              */
    int32_t lo_thresh;      /* 2000                                                */
    int32_t shift;          /* 1000    subtracted from both ends when reporting    */
    double  std_scale;      /* 0.5                                                 */
    int32_t lim_low;        /* 0       scale_outliers limits (:329-332)            */
    int32_t lim_hi;         /* 1200                                                */
} sk_roll_params;
/* xy[2r], xy[2r+1] = the reported pair of read r when found[r] != 0. */
int sk_drna_roll_batch_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                           const sk_roll_params *p, int32_t *xy, int32_t *found);
/* Device-resident forms of the two dRNA_segmenter.py branches (same kernels; d_sig, d_len and the outputs are device
 * pointers, every len[r] is clamped into [0, stride] by the kernels; nothing is synchronised -- sk_sync()).  What
 * bench.py times at 250 000 reads per call.  Reference: dRNA_segmenter.py:85-176 (slow5 branch), :272-326 (--signal). */
int sk_drna_segment_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                            const sk_drna_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs);
int sk_drna_roll_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                         const sk_roll_params *p, int32_t *d_xy, int32_t *d_found);

/* ---- MotifSeq path ---------------------------------------------------- */
/* Replaces, per read r: scale_outliers (MotifSeq.py:274,317-324), medmad
 * (:192-200) or zscale (:186-191), then mlpy.dtw_subsequence(motif, sig)
 * (:437) reduced to what the caller uses (:438-439): dist, start, end.
 * motif: nmotif float64 points (model[name], MotifSeq.py:354-428). */
int sk_motifseq_batch_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                          const double *motif, int32_t nmotif, int32_t scale_mode,
                          int32_t scale_low, int32_t scale_hi, sk_hit *out);
/* Several motifs against the same reads -- the `for name in m_order` loop of MotifSeq.py:436:
 * motif k is motifs[motif_off[k] .. motif_off[k+1]); out is [nmotifs][nreads].  Filter and
 * statistics run once. */
int sk_motifseq_multi_batch_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                                const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                                int32_t scale_mode, int32_t scale_low, int32_t scale_hi, sk_hit *out);
int sk_motifseq_batch_f64(const double *sig, const int64_t *off, int32_t nreads,
                          const double *motif, int32_t nmotif, int32_t scale_mode,
                          int32_t scale_low, int32_t scale_hi, sk_hit *out);
/* Several motifs against the same ragged float64 batch -- the `for name in m_order` loop of MotifSeq.py:436 on pA
 * input: the batch is staged and filtered once, one DTW launch set per motif.  motif k = motifs[motif_off[k] ..
 * motif_off[k+1]); out is [nmotifs][nreads]. */
int sk_motifseq_multi_batch_f64(const double *sig, const int64_t *off, int32_t nreads,
                                const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                                int32_t scale_mode, int32_t scale_low, int32_t scale_hi, sk_hit *out);
/* sk_motifseq_multi_batch_f64 for int32 centi-units (see sk_segment_batch_centi_len; MotifSeq.py:270) */
int sk_motifseq_multi_batch_centi(const int32_t *centi, const int64_t *off, int32_t nreads,
                                  const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                                  int32_t scale_mode, int32_t scale_low, int32_t scale_hi, sk_hit *out);
/* device-resident form (d_sig, d_len, d_out device; motif host). */
int sk_motifseq_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                        const double *motif, int32_t nmotif, int32_t scale_mode,
                        int32_t scale_low, int32_t scale_hi, sk_hit *d_out);
/* device-resident forms of the multi-motif and float64 entry points (motifs / motif_off host; d_out is
 * [nmotifs][nreads]; d_off zero based, total = d_off[nreads], max_len >= the longest read). */
int sk_motifseq_multi_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                              int32_t scale_mode, int32_t scale_low, int32_t scale_hi, sk_hit *d_out);
int sk_motifseq_dev_f64(const double *d_sig, const int64_t *d_off, int32_t nreads, int64_t total, int64_t max_len,
                        const double *motif, int32_t nmotif, int32_t scale_mode,
                        int32_t scale_low, int32_t scale_hi, sk_hit *d_out);

/* Hit lists: up to max_hits non-overlapping matches per read and motif, not only the first argmin of
 * cost[-1, :] that MotifSeq.py:437-439 keeps (view_region plots that whole row, :506-513).  For read r
 * (filtered and normalised as above) and motif x of N points, d_j = cost[-1, j] and s_j = the column where
 * subsequence_path's back-trace from (N-1, j) reaches row 0 (diagonal, then j-1, then i-1).  Greedy:
 * max_hits times, among the columns j with d_j <= max_dist whose [s_j, j] is disjoint from every interval
 * taken so far, take the smallest d_j (ties: the smallest j); stop when there is none.  Hit 1 is the record
 * of sk_motifseq_multi_batch_i16 bit for bit; dist never decreases with rank.
 * out is [nmotifs][nreads][max_hits] (dist, start, end, n, flags), count [nmotifs][nreads]; unused slots
 * hold dist NaN, start = end = -1 and the read's n and flags.  Reads flagged SK_FLAG_EMPTY or
 * SK_FLAG_DEGENERATE have count 0.  max_hits outside 1..64 or a NaN max_dist (+inf: no limit): SK_ERR_INVALID. */
int sk_motifseq_hits_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                         const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                         int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                         int32_t *count);
/* the same on ragged float64 reads (pA input): read r = sig[off[r] .. off[r+1]) */
int sk_motifseq_hits_f64(const double *sig, const int64_t *off, int32_t nreads,
                         const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                         int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                         int32_t *count);
/* sk_motifseq_hits_f64 for int32 centi-units (value / 100 made on the device, as sk_motifseq_multi_batch_centi) */
int sk_motifseq_hits_centi(const int32_t *centi, const int64_t *off, int32_t nreads,
                           const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                           int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                           int32_t *count);
/* device-resident form (d_sig, d_len, d_out, d_count device; motifs / motif_off host) */
int sk_motifseq_hits_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                             const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                             int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *d_out,
                             int32_t *d_count);

/* Alignment paths: the hit list, and per hit which samples belong to which point of the motif.  mlpy's
 * dtw_subsequence returns the whole warping path (MotifSeq.py:437); the path of a hit (dist, start, end) is
 * subsequence_path's back-trace in the full N x n matrix from (N-1, end): while i > 0 -- at j == 0 up, else
 * with mc = min3(up, diag, left): diagonal if diag == mc, else left if left == mc, else up -- reversed.  In it
 * motif point i covers one contiguous column range [a_i, b_i], with a_0 = b_0 = start, b_{N-1} = end and
 * a_{i+1} = b_i or b_i + 1; the path is (i, j) for j = a_i .. b_i, i ascending.
 * spans holds (a_i, b_i) per hit, in filtered coordinates like start / end: motif k's block begins at
 * 2 * max_hits * nreads * motif_off[k] int32, inside it [read][hit][N_k][2].  A hit without a path -- an unused
 * slot, a read flagged SK_FLAG_EMPTY or SK_FLAG_DEGENERATE, a failed self-check -- has all spans -1.
 * out / count: exactly what the sk_motifseq_hits_* twin returns; the other arguments are its own. */
int sk_motifseq_paths_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                          const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                          int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                          int32_t *count, int32_t *spans);
int sk_motifseq_paths_f64(const double *sig, const int64_t *off, int32_t nreads,
                          const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                          int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                          int32_t *count, int32_t *spans);
int sk_motifseq_paths_centi(const int32_t *centi, const int64_t *off, int32_t nreads,
                            const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                            int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                            int32_t *count, int32_t *spans);
/* device-resident form (d_sig, d_len, d_out, d_count, d_spans device; motifs / motif_off host) */
int sk_motifseq_paths_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                              int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *d_out,
                              int32_t *d_count, int32_t *d_spans);
/* Every path is checked on the device: the kernel recomputes the DTW on the window y[start .. end] alone, whose
 * corner must carry the bits of the hit's dist and whose back-trace must end on (0, start).  A hit that fails
 * gets spans -1 and is counted here, for the calling thread's last paths call (-1: none yet).  A healthy build
 * reports 0. */
int sk_last_path_mismatches(void);

/* Events: the hit list, and per hit and motif point what the signal did in the samples the path gives that point --
 * the row an eventalign / resquiggle table has per base.  With y the read's filtered, normalised samples (the values
 * the DTW compares, as sk_normalise_* returns them), x the motif and w = y[a_i .. b_i] the span of point i:
 *   sum    = np.sum(w)                 (np.add.reduce's order, as sk_bg_rec documents it: serial below 8 samples,
 *                                       eight accumulators up to 128, the pairwise split above, buffers of 8 192)
 *   std    = np.std(w)                 (ddof 0, two passes, the same order; one sample: 0.0)
 *   cost   = np.sum(np.abs(x[i] - w))  (this point's share of the hit's distance; the same order)
 *   start  = a_i, dwell = b_i - a_i + 1       (filtered coordinates)
 * bit for bit what numpy gives.  The mean is not stored: sum / dwell has the bits of np.mean(w).  A column two
 * consecutive points share (a_{i+1} == b_i) counts for both.  A hit without a path -- an unused slot, a read flagged
 * SK_FLAG_EMPTY or SK_FLAG_DEGENERATE, a failed self-check -- has sum = std = cost = NaN, start = -1, dwell = 0 in
 * all its records. */
typedef struct sk_event {           /* 32 bytes */
    double  sum;
    double  std;
    double  cost;
    int32_t start;
    int32_t dwell;
} sk_event;
/* events follows the layout of spans: motif k's block begins at max_hits * nreads * motif_off[k] records, inside it
 * [read][hit][N_k].  out / count: exactly what the sk_motifseq_hits_* twin returns; the other arguments are those of
 * the sk_motifseq_paths_* twin, and sk_last_path_mismatches() counts for an events call as for a paths call.  A NULL
 * events is SK_ERR_INVALID. */
int sk_motifseq_events_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                           const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                           int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                           int32_t *count, sk_event *events);
int sk_motifseq_events_f64(const double *sig, const int64_t *off, int32_t nreads,
                           const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                           int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                           int32_t *count, sk_event *events);
int sk_motifseq_events_centi(const int32_t *centi, const int64_t *off, int32_t nreads,
                             const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                             int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                             int32_t *count, sk_event *events);
/* device-resident form (d_sig, d_len, d_out, d_count, d_events device; motifs / motif_off host) */
int sk_motifseq_events_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                               const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                               int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *d_out,
                               int32_t *d_count, sk_event *d_events);

/* Pooled model: the events of nhits hits against one motif of N points (ev is [nhits][N], in any order the caller
 * likes -- the hits of many reads, of many calls) reduced to one record per motif point.  A hit is selected when
 * use[h] != 0 (use NULL: every hit) and it has a path (dwell > 0 in its first record; the records of a hit have a
 * path or none).  With the selected records of point i taken as contiguous float64 arrays in hit order -- sum_col,
 * std_col, cost_col, dwell_col -- and total_dwell the exact int64 sum of dwell_col, one record holds, bit for bit
 * what numpy gives:
 *   level      = np.sum(sum_col) / total_dwell   (sample weighted: one update of DTW barycentre averaging)
 *   level_sd   = np.std(sum_col / dwell_col)     (spread of the event means over the hits)
 *   sd_mean    = np.mean(std_col)                (noise inside an event)
 *   dwell_mean = total_dwell / hits
 *   dwell_sd   = np.std(dwell_col.astype(np.float64))
 *   cost_mean  = np.mean(cost_col)
 *   hits       = selected hits; 0: the six doubles are NaN
 * nhits above 2 147 418 112 or N < 1: SK_ERR_INVALID. */
typedef struct sk_pool_rec {        /* 56 bytes */
    double  level;
    double  level_sd;
    double  sd_mean;
    double  dwell_mean;
    double  dwell_sd;
    double  cost_mean;
    int32_t hits;
    int32_t pad;                    /* 0 */
} sk_pool_rec;
int sk_events_pool(const sk_event *ev, const uint8_t *use, int64_t nhits, int32_t N, sk_pool_rec *out);
/* device-resident form (d_ev, d_use, d_out device) */
int sk_events_pool_dev(const sk_event *d_ev, const uint8_t *d_use, int64_t nhits, int32_t N, sk_pool_rec *d_out);

/* Read background: the hit list, and per read and motif the statistics of the whole last DTW row the hits were
 * taken from.  view_region draws a hit against its read's own row of distance scores (MotifSeq.py:507-513:
 * M = np.mean(cost[-1,]), S = np.std(cost[-1,]), lines at M and M - S); with d = cost[-1, :] of motif k against
 * read r (its n filtered, normalised samples -- the row the hit list selects from), one record holds, bit for bit
 * what numpy gives on that row:
 *   mean   = np.mean(d)                 (np.add.reduce's order: serial over chunks of 8 192, pairwise inside)
 *   std    = np.std(d)                  (ddof 0, two passes: sqrt(sum((d - mean)^2) / n), the same order)
 *   median = np.median(d)               (even n: (a + b) / 2 of the two middle values)
 *   mad    = np.median(np.abs(d - median))          (not multiplied by 1.4826)
 *   below  = number of columns with d[j] < mean - std   (one float64 subtraction, strict compare; :510)
 *   n      = columns of the row = the read's filtered length
 * A read flagged SK_FLAG_EMPTY or SK_FLAG_DEGENERATE has four NaNs, below = -1 and its n.  Scores of a hit
 * against its read are left to the caller: local_Z = (dist - mean) / std, robust_Z = (dist - median) /
 * (mad * 1.4826), the constant of MotifSeq.py:192-200. */
typedef struct sk_bg_rec {          /* 48 bytes */
    double  mean;
    double  std;
    double  median;
    double  mad;
    int32_t below;
    int32_t n;
    int32_t reserved[2];            /* 0 */
} sk_bg_rec;
/* bg is [nmotifs][nreads]; out / count: exactly what the sk_motifseq_hits_* twin returns; the other arguments are
 * its own.  A NULL bg is SK_ERR_INVALID. */
int sk_motifseq_background_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                               const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                               int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                               int32_t *count, sk_bg_rec *bg);
int sk_motifseq_background_f64(const double *sig, const int64_t *off, int32_t nreads,
                               const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                               int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                               int32_t *count, sk_bg_rec *bg);
int sk_motifseq_background_centi(const int32_t *centi, const int64_t *off, int32_t nreads,
                                 const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                                 int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                                 int32_t *count, sk_bg_rec *bg);
/* device-resident form (d_sig, d_len, d_out, d_count, d_bg device; motifs / motif_off host) */
int sk_motifseq_background_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                                   const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                                   int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *d_out,
                                   int32_t *d_count, sk_bg_rec *d_bg);

/* Motif panel inside a search region: which of K known signals (barcodes, adapters, primers) sits at a known place of
 * the read.  Region: read r's raw samples are cut as the Python slice raw[begin:end] BEFORE scale_outliers -- negative
 * values count from the end of the read, end = INT32_MAX means "to the end", everything resolved as
 * slice(begin, end).indices(len[r]) resolves it (an empty result is allowed: SK_FLAG_EMPTY); win (NULL, or [nreads][2])
 * gives every read its own (begin, end) instead, e.g. segmenter-derived cuts.  What follows is the reference run on the
 * sliced read: the filter (MotifSeq.py:317-324), medmad or zscale over the slice (:186-200), dtw_subsequence (:437);
 * start / end / n index the slice's filtered samples, from[r] is the resolved raw begin (what --after_stall prints as
 * search_from).  Records: motif k's (dist, start, end, n, flags) of read r is bit for bit what
 * sk_motifseq_multi_batch_i16 returns for the sliced rows.  Ranking: score[k] = (dist_k - mean[k]) / sd[k], one
 * correctly rounded FP64 subtraction and one division -- the Z-score of MotifSeq.py:441-443, mean = slope * L_k +
 * intercept and sd = mean * std_const made by the caller; best = the smallest score (ties: the smallest k), second =
 * the best of the rest; a NaN score is never ranked.  A read flagged SK_FLAG_EMPTY or SK_FLAG_DEGENERATE has
 * best = second = -1 and NaN scores; with one motif second = -1 and score_second is NaN. */
typedef struct sk_panel_rec {   /* 48 bytes, one per read */
    int32_t best, second;       /* motif indices, -1: none                                              */
    double  score_best, score_second;
    sk_hit  hit;                /* the best motif's record (dist NaN, start = end = -1, the read's n and flags when best == -1) */
} sk_panel_rec;
/* out [nreads]; from [nreads] or NULL; all [nmotifs][nreads] (every motif's record) or NULL.  Region alone is this call
 * with one motif and `all`.  SK_ERR_INVALID: nmotifs outside 1..256, an empty motif, sd[k] == 0, a non-finite mean or
 * sd, a win row whose resolved begin lies behind its end (unless both were cut to the read, as a slice cuts them), NULL
 * where a pointer is required.  Large calls are moved in sub-batches like the other host entry points. */
int sk_motifseq_panel_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                          int32_t begin, int32_t end, const int32_t *win,
                          const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                          const double *mean, const double *sd,
                          int32_t scale_mode, int32_t scale_low, int32_t scale_hi,
                          sk_panel_rec *out, int32_t *from, sk_hit *all);
/* device-resident form: d_sig, d_len, d_win, d_out, d_from, d_all device; motifs / motif_off / mean / sd host.  len[r]
 * is clamped into [0, stride]; a d_win row whose resolved begin lies behind its end is an empty window (the library
 * cannot look).  Nothing is synchronised. */
int sk_motifseq_panel_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              int32_t begin, int32_t end, const int32_t *d_win,
                              const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                              const double *mean, const double *sd,
                              int32_t scale_mode, int32_t scale_low, int32_t scale_hi,
                              sk_panel_rec *d_out, int32_t *d_from, sk_hit *d_all);
/* ragged float64 reads (pA input): read r = sig[off[r] .. off[r+1]) */
int sk_motifseq_panel_f64(const double *sig, const int64_t *off, int32_t nreads,
                          int32_t begin, int32_t end, const int32_t *win,
                          const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                          const double *mean, const double *sd,
                          int32_t scale_mode, int32_t scale_low, int32_t scale_hi,
                          sk_panel_rec *out, int32_t *from, sk_hit *all);
/* The gather alone (k_region_rows): the window rows of the region, for callers that hand them to another entry point
 * (hit lists, paths).  rows [nreads][wstride] (zero padded), wlen [nreads], from [nreads] or NULL; wstride: a multiple
 * of 8 that holds the longest resolved slice (SK_ERR_INVALID otherwise).  win as above. */
int sk_region_rows_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                       int32_t begin, int32_t end, const int32_t *win, int64_t wstride,
                       int16_t *rows, int32_t *wlen, int32_t *from);

/* The mlpy boundary itself: dtw_subsequence(x, y) on already-normalised
 * float64 signals (MotifSeq.py:437).  Batch form: read r is y[off[r]..off[r+1]). */
int sk_dtw_subsequence_batch(const double *x, int32_t nx, const double *y, const int64_t *off,
                             int32_t nreads, sk_hit *out);
/* Single pair, the reference's call shape.  cost_last_row (may be NULL, else
 * ny doubles) receives cost[-1, :] (what view_region plots, MotifSeq.py:507). */
int sk_dtw_subsequence(const double *x, int32_t nx, const double *y, int32_t ny,
                       double *dist, int32_t *start, int32_t *end, double *cost_last_row);
/* Single pair with the path of its match: spans [nx][2] as above (mlpy's third return value). */
int sk_dtw_subsequence_path(const double *x, int32_t nx, const double *y, int32_t ny,
                            double *dist, int32_t *start, int32_t *end, int32_t *spans);

/* ---- DTW over a pair list: a query of its own per pair, shared targets --------------------------------------------
 * The pool is ragged float64: sequence s = values[off[s] .. off[s+1]), nseq sequences, taken as given (no filter, no
 * normalisation).  A pair names two sequences of the pool: the query and the target.  A sequence may be the query of
 * some pairs and the target of others; (i, i) is allowed.  out [npairs], in the caller's order.
 *   SK_PAIRS_SUBSEQUENCE  the record of pair p is what sk_dtw_subsequence(values[query], values[target]) returns: free
 *       start and end along the target, first argmin of the last row, start by the back-trace order diagonal, j-1,
 *       i-1; n = the target's length.
 *   SK_PAIRS_GLOBAL  both ends pinned: D[0][0] = |x0 - y0|, D[0][j] = D[0][j-1] + |x0 - yj|, D[i][0] = D[i-1][0] +
 *       |xi - y0|, inside |xi - yj| + min3 as above; dist = D[N-1][M-1], start = 0, end = M - 1, n = M.  This is mlpy's
 *       dtw_std(x, y, dist_only=True) as published; no mlpy build was compared against.  The distance is symmetric bit
 *       for bit (the transposed path adds the same cells in the same order).
 * An empty target gives dist NaN, start = end = -1 and SK_FLAG_EMPTY.  SK_ERR_INVALID (with the pair named, nothing
 * launched, no record written): an empty query, an index outside [0, nseq).  SK_ERR_UNSUPPORTED: a query of more than
 * 1 024 points (the pair named), npairs above 2^27.  npairs == 0 returns SK_OK.  Non-finite values: unspecified.
 * Every distinct query is laid out once however many pairs use it; pairs whose queries share a lane layout are swept
 * by one launch, four pairs to a wavefront for short queries in large calls. */
enum { SK_PAIRS_SUBSEQUENCE = 0, SK_PAIRS_GLOBAL = 1 };
typedef struct sk_pair { int32_t query, target; } sk_pair;     /* 8 bytes */
int sk_dtw_pairs(const double *values, const int64_t *off, int32_t nseq,
                 const sk_pair *pairs, int64_t npairs, int32_t mode, sk_hit *out);
/* device-resident form: d_values and d_out on the device; off and pairs on the host (the plan needs the lengths).
 * Nothing is synchronised after the launches. */
int sk_dtw_pairs_dev(const double *d_values, const int64_t *off, int32_t nseq,
                     const sk_pair *pairs, int64_t npairs, int32_t mode, sk_hit *d_out);

/* Warping paths of a pair list: WHICH target points every query point covers (the resquiggle / eventalign assignment).
 * For pair p = (q, t) with N = len(q), M = len(t) the path is written as spans, int32 [N][2]: query point i covers the
 * target points [a_i, b_i], in the coordinates of the target -- the meaning of sk_motifseq_paths_*.  The spans of pair p
 * start at row span_off[p] = sum of N_k over the pairs k < p of one int32 [sum N][2] array: list order, a query used by
 * several pairs counted once per pair (the caller derives span_off from off and pairs).
 *   SK_PAIRS_SUBSEQUENCE  mlpy's subsequence_path from (N-1, end): while i > 0 -- at j == 0 up; else diagonal if it
 *       equals min3(up, diag, left), else left if it does, else up.  a_0 = b_0 = start, b_{N-1} = end.
 *   SK_PAIRS_GLOBAL  mlpy's path() from (N-1, M-1): while i > 0 || j > 0 -- at i == 0 left, at j == 0 up, else the same
 *       order.  Row 0 covers [0, b_0]: a_0 = 0, b_{N-1} = M - 1.  This is the path dtw_std(x, y, dist_only=False)
 *       returns in mlpy as published; no mlpy build was compared against.
 * In both modes a_i <= b_i and a_{i+1} is b_i or b_i + 1.
 * have_records == 0: the records are computed first -- byte for byte what sk_dtw_pairs writes -- stored to `records`,
 * then traced.  have_records == 1: `records` is input and names the window [start, end] of the target to trace, e.g.
 * the merged records of a tiled search, in whole-target coordinates, against the whole targets.  Subsequence mode uses
 * start / end / dist; global mode requires start == 0 and end == M - 1.
 * Self-check per pair: the DTW recomputed on the window ends, in its corner, on the bits of the record's dist, and the
 * trace ends on the record's start.  A pair that fails -- or whose record has start / end outside [0, M), end < start,
 * or, in global mode, another window than the whole target -- gets spans -1 and is counted by
 * sk_last_path_mismatches(); nothing outside the target is ever read.  A record with NaN dist or SK_FLAG_EMPTY gets
 * spans -1 and is not counted.
 * Refusals: those of sk_dtw_pairs, same codes and messages, nothing written; a NULL spans is SK_ERR_INVALID.
 * npairs == 0 returns SK_OK. */
int sk_dtw_pairs_paths(const double *values, const int64_t *off, int32_t nseq,
                       const sk_pair *pairs, int64_t npairs, int32_t mode,
                       sk_hit *records, int32_t have_records, int32_t *spans);
/* device-resident form: d_values, d_records and d_spans on the device; off and pairs on the host.  The call
 * synchronises once between its two launches (the second tier's scratch is sized from the first); nothing is
 * synchronised after them. */
int sk_dtw_pairs_paths_dev(const double *d_values, const int64_t *off, int32_t nseq,
                           const sk_pair *pairs, int64_t npairs, int32_t mode,
                           sk_hit *d_records, int32_t have_records, int32_t *d_spans);
/* The tiers of the last such call (diagnostic): pairs whose direction words or window did not fit the LDS tier, the
 * bytes of one scratch slab (sized from those pairs), the wavefronts that shared them.  Any pointer may be NULL. */
int sk_last_pair_paths_tiers(int64_t *listed, int64_t *slab_bytes, int64_t *waves);

/* Adaptive-band DTW over a pair list: records and warping paths of WHOLE reads in one pass.  The pool, the pair list and
 * the order of the results are those of sk_dtw_pairs; the start is pinned to cell (0, 0), the end is pinned to
 * (N-1, M-1) (SK_BAND_PINNED) or free along the last row (SK_BAND_FREE).  Instead of the N x M matrix one wavefront
 * sweeps the pair's anti-diagonals inside a band of `band` = W cells (64, 128 or 256) that follows the path (the
 * Suzuki-Kasahara scheme): (N + M - 1) * W cells per pair and W / 4 bytes of direction words per anti-diagonal.
 *   Band b = 0 .. N + M - 2 has a lower-left corner (I_b, J_b), (I_0, J_0) = (W/2, -W/2); offset o = 0 .. W - 1 of band b
 *   is the cell (I_b - o, J_b + o).  A cell outside the matrix holds +inf.  D(0, 0) = |x0 - y0|; elsewhere up = D(i-1, j)
 *   and left = D(i, j-1) are read from band b - 1 and diag = D(i-1, j-1) from band b - 2 at the offsets of those cells,
 *   +inf when the offset is outside [0, W).  m1 = left < diag ? left : diag; m = up < m1 ? up : m1; D = |x_i - y_j| + m;
 *   the stored direction is up if up < m1, else left if left < diag, else diagonal (mlpy's back-trace order).
 *   After band b, with ll = D_b[0] and ur = D_b[W-1]: ur < ll moves right (J + 1), ll < ur moves down (I + 1), anything
 *   else (equal, both +inf, a NaN) moves right for even b and down for odd b.
 *   SK_BAND_PINNED  dist = D(N-1, M-1) if the last band holds that cell, else +inf; end = M - 1.
 *   SK_BAND_FREE    over the bands in ascending order, the first strictly smallest D of row N - 1; end = its column.
 *   start = 0, n = M.  dist == +inf: the band lost the corner -- dist = +inf, start = end = -1, SK_FLAG_BAND_LOST.
 * When N <= W/2 and M <= W/2 every cell is in its band: the record is that of SK_PAIRS_GLOBAL (free end: the first argmin
 * of the full matrix's last row) bit for bit.  Otherwise dist is >= the full matrix's and may be larger.
 * spans (NULL: records only): int32 [sum N][2] with the meaning and layout of sk_dtw_pairs_paths -- the stored directions
 * followed from (N-1, end) to (0, 0); a_0 = 0, b_{N-1} = end.  Self-check per pair: the walk stays inside the band and
 * ends on offset W/2 of band 0; a pair that fails, or lost the corner, gets spans -1 and is counted by
 * sk_last_path_mismatches().  An empty target gives dist NaN, start = end = -1, SK_FLAG_EMPTY, spans -1, not counted.
 * Refusals (checked before anything else, nothing written): band not 64 / 128 / 256, an unknown end mode, and those of
 * sk_dtw_pairs with the same codes and messages, but for the lengths: 1 <= N <= 2^20 and M <= 2^20, SK_ERR_UNSUPPORTED
 * above with the pair named.  Memory: one slab of ceil(steps * W / 1024) * 256 + ceil(steps / 64) * 8 + 8 bytes per
 * wavefront, steps = N + M - 1 of the longest listed pair; the slabs of a call take at most 8 GiB (that bounds the
 * wavefronts, otherwise as many as the device holds at a time); a slab above the budget is SK_ERR_NOMEM.  npairs == 0
 * returns SK_OK. */
enum { SK_BAND_PINNED = 0, SK_BAND_FREE = 1 };
enum { SK_FLAG_BAND_LOST = 16 };   /* sk_hit.flags of sk_dtw_band: the band lost the end cell (dist = +inf) */
int sk_dtw_band(const double *values, const int64_t *off, int32_t nseq,
                const sk_pair *pairs, int64_t npairs, int32_t band, int32_t end_mode,
                sk_hit *records, int32_t *spans /* NULL: records only */);
/* device-resident form: d_values, d_records and d_spans on the device; off and pairs on the host.  One launch; nothing
 * is synchronised after it. */
int sk_dtw_band_dev(const double *d_values, const int64_t *off, int32_t nseq,
                    const sk_pair *pairs, int64_t npairs, int32_t band, int32_t end_mode,
                    sk_hit *d_records, int32_t *d_spans);
/* The plan of the last such call (diagnostic): bytes of one slab (0 for a records-only call), the wavefronts of the
 * launch, N + M - 1 of the longest listed pair.  Any pointer may be NULL. */
int sk_last_band_plan(int64_t *slab_bytes, int64_t *waves, int64_t *steps_max);

/* The same call in mlpy's own C arithmetic for inputs that hold inf / nan -- `min3` as "a; if (b < m) m = b; if (c < m)
 * m = c", fabs, np.argmin's first-NaN rule, the back-trace of subsequence_path, all evaluated literally by one GPU lane
 * over the full cost matrix.  medmad of a read whose MAD is 0 divides by zero (MotifSeq.py:196-199) and the reference
 * prints whatever mlpy makes of the result; `MotifSeq.py --strict-compat` prints the same row through this entry. */
int sk_dtw_subsequence_cref(const double *x, int32_t nx, const double *y, int32_t ny,
                            double *dist, int32_t *start, int32_t *end);

/* Normalised signal of one read exactly as the reference hands it to
 * dtw_subsequence (used by MotifSeq -x/--sig_extract, MotifSeq.py:446-447).
 * out must hold len doubles; *n_out receives the filtered length. */
int sk_normalise_i16(const int16_t *sig, int32_t len, int32_t scale_mode,
                     int32_t scale_low, int32_t scale_hi, double *out, int32_t *n_out);
int sk_normalise_f64(const double *sig, int32_t len, int32_t scale_mode,
                     int32_t scale_low, int32_t scale_hi, double *out, int32_t *n_out);

/* ---- TSV ingest (host code; no GPU needed) ------------------------------ */
/* Native replacement of the per-line split + int()/float() loops that feed the hot path
 * (segmenter.py:192-201 reads columns 4.., MotifSeq.py:265-270 columns 8..; layout written by
 * SquigglePull.py:243-253).  Three calls: count lines, count data tokens per line (caller turns
 * them into offsets), parse into one flat float64 array.  Conversion is exactly float()'s for
 * plain decimal tokens; lines with any other token get SK_TSV_SLOW and should be parsed by the
 * caller the slow way.  Call sk_tsv_count_lines first on every new content of a buffer: it builds the
 * per-thread line index the other calls reuse (they re-check a cached index against the bytes -- every line
 * start must follow a newline, the line count must match -- and rebuild it otherwise). */
enum {
    SK_TSV_ALLINT   = 1,   /* every data token is [+-]digits                                  */
    SK_TSV_ANY      = 2,   /* some value is non-zero (the reference skips reads where none is) */
    SK_TSV_FIRSTDOT = 4,   /* the first data token contains '.' (segmenter.py:198 picks float) */
    SK_TSV_SLOW     = 8,   /* a token is outside the plain grammar: use the fallback parser    */
    SK_TSV_SHORT    = 16,  /* the line has no data column at all                               */
    SK_TSV_CENTI    = 32   /* sk_tsv_parse_centi: every data token has at most two decimals     */
};
int64_t sk_tsv_count_lines(const char *buf, size_t len);
int sk_tsv_count_tokens(const char *buf, size_t len, int32_t start_col, int64_t nlines, int64_t *ntok,
                        int32_t nthreads);
int sk_tsv_parse(const char *buf, size_t len, int32_t start_col, int64_t nlines, const int64_t *off,
                 double *values, int64_t *name_off, int32_t *name_len, int64_t *id_off, int32_t *id_len,
                 int32_t *flags, int32_t nthreads);

/* Decimal lines as int32 centi-units (round 6): SquigglePull's default output is np.round(pA, 2)
 * (SquigglePull.py:183-189,222), and float("ddd.dd") == (double)ddddd / 100.0 bit for bit, so a line whose data tokens
 * all have at most two decimals travels as int32 (half the bytes, one pass) and becomes float64 on the device.  Same
 * layout as sk_tsv_parse (values[off[i] .. off[i+1]) = line i); flags[i] & SK_TSV_CENTI says line i's values are valid --
 * a chunk with any line without it goes through sk_tsv_parse instead.  Replaces the float() loops of
 * segmenter.py:198-199 / MotifSeq.py:270 for such lines. */
int sk_tsv_parse_centi(const char *buf, size_t len, int32_t start_col, int64_t nlines, const int64_t *off,
                       int32_t *values, int64_t *name_off, int32_t *name_len, int64_t *id_off, int32_t *id_len,
                       int32_t *flags, int32_t nthreads);

/* Integer lines straight into int16 rows (the raw-signal TSVs SquigglePull writes): rows[i * stride ..] = line i's
 * data tokens, nsamp[i] their number.  flags[i] has SK_TSV_ALLINT only if every data token is [+-]digits, fits
 * int16 and the line has at most `stride` of them (the row is valid only then); other lines get SK_TSV_SLOW /
 * SK_TSV_SHORT and go the general way.  line_off[i] (nlines + 1 entries) = byte offset of line i. */
int sk_tsv_parse_i16(const char *buf, size_t len, int32_t start_col, int64_t nlines, int64_t stride, int16_t *rows,
                     int32_t *nsamp, int64_t *name_off, int32_t *name_len, int64_t *id_off, int32_t *id_len,
                     int32_t *flags, int64_t *line_off, int32_t nthreads);

/* ---- result tables as text / BLOW5 ingest (host code; no GPU needed) ------ */
/* The rows the command-line tools print (MotifSeq.py:446-449: 12 tab-separated columns per hit; segmenter.py:222-227:
 * name <TAB> s0,e0,s1,e1...) formatted on all cores: columns of strings, int32, float64 -- floats exactly as Python's
 * "{}".format(float) / repr() writes them -- or comma-joined int32 lists.  Rows with skip[i] != 0 are left out.
 * Returns a malloc'ed buffer of *out_len bytes (free with sk_fmt_free), NULL on failure. */
enum { SK_FMT_STR = 0, SK_FMT_I32 = 1, SK_FMT_F64 = 2, SK_FMT_CONST = 3, SK_FMT_I32LIST = 4, SK_FMT_STRSPAN = 5 };
typedef struct sk_fmt_col {
    int32_t        kind;     /* SK_FMT_*                                                                    */
    const void    *data;     /* STR / CONST: bytes; I32 / I32LIST: int32[]; F64: double[]                   */
    const int64_t *off;      /* STR / I32LIST: nrows + 1 offsets into data; CONST: off[0..1]; STRSPAN: [nrows][2]
                                = first / one-past-last byte of row i's string in data; else unused         */
} sk_fmt_col;
void *sk_fmt_rows(int64_t nrows, int32_t ncols, const sk_fmt_col *cols, const uint8_t *skip, int32_t nthreads,
                  int64_t *out_len);
void  sk_fmt_free(void *p);
/* out[i] = the standard normal CDF of z[i], the very double scipy.special.ndtr returns (MotifSeq.py:444 prints
 * scipy.stats.norm.cdf(z) digit for digit): the Cephes ndtr, restated in csrc/sk_io.cpp. */
void  sk_ndtr(const double *z, double *out, int64_t n);

/* BLOW5 (binary SLOW5: what the reference reads through pyslow5, segmenter.py:321-396, dRNA_segmenter.py:85-100).
 * sk_blow5_index walks the records of a file image from byte `first` (just behind the ASCII header): payload offset
 * and size of up to `cap` records; returns the number of records in the file (call with cap = 0 to count).
 * sk_blow5_index_some is the same walk for at most max_rec records from byte `pos`; *next_pos = where the next call
 * continues, fewer than max_rec records returned = end of the file (a reader indexes chunk by chunk).
 * sk_blow5_rows_i16 decodes records (comp: 0 = stored, 1 = zlib) into int16 rows of `stride` samples on all cores:
 * nsamp[i] samples, ids[i * id_width ..] the read id (NUL padded; NULL to skip), calib[3 i ..] = digitisation, offset,
 * range (NULL to skip); flags[i]: 1 = longer than a row (truncated to stride), 2 = unreadable record (also: offset /
 * size outside the `len` bytes of buf, a zlib record that inflates past 256x its size), 4 = id cut to id_width.
 * Both index calls return SK_ERR_INVALID for a file cut inside a record or a size field, or with anything but the
 * end marker behind the last record. */
int64_t sk_blow5_index(const void *buf, int64_t len, int64_t first, int64_t *rec_off, int64_t *rec_size, int64_t cap);
int64_t sk_blow5_index_some(const void *buf, int64_t len, int64_t pos, int64_t max_rec, int64_t *rec_off,
                            int64_t *rec_size, int64_t *next_pos);
int sk_blow5_rows_i16(const void *buf, int64_t len, const int64_t *rec_off, const int64_t *rec_size, int64_t nrec,
                      int32_t comp, int64_t stride, int16_t *rows, int32_t *nsamp, char *ids, int32_t id_width, double *calib,
                      int32_t *flags, int32_t nthreads);

/* ---- multi-GPU: the final gather of result records (RCCL over xGMI) ------ */
/* The reference's per-read loops (segmenter.py:189-230, MotifSeq.py:261-298) carry no state from one read
 * to the next, so N GPUs take contiguous blocks of the reads with no data-path collective; the one exchange
 * is an all-gather of the fixed-size records at the end.  librccl.so is loaded on first use; when it (or a
 * communicator) is not available these return SK_ERR_UNSUPPORTED and the caller concatenates the shards on
 * the host.  One communicator per device; the calls act on the calling thread's bound device.
 *   one process, one thread per GPU:   sk_comm_init_all(devices, n)  once, from any thread
 *   one process per GPU:               rank 0: sk_comm_unique_id(id) -> hand the 128 bytes to every rank;
 *                                      every rank: sk_init(dev); sk_comm_init_rank(id, nranks, rank)        */
int sk_comm_unique_id(void *id128);
int sk_comm_init_rank(const void *id128, int nranks, int rank);
int sk_comm_init_all(const int *devices, int ndev);
int sk_comm_info(int *nranks, int *rank);      /* what RCCL reports for this device's communicator */
/* d_recv[nranks * bytes] <- every rank's d_send[bytes], rank order; enqueued on the device's stream */
int sk_comm_allgather_dev(const void *d_send, void *d_recv, size_t bytes);
/* the same for small host buffers (timings, a barrier); synchronous */
int sk_comm_allgather_host(const void *send, void *recv, size_t bytes);
int sk_comm_destroy(void);

/* ---- tuning switches --------------------------------------------------- */
/* Every environment switch the library reads, as text: one line per switch, "name<TAB>values the parity test flips it
 * to<TAB>description".  None changes results; all are ignored unless SK_TUNING=1 is set too.  Returns the bytes needed
 * (including the terminating NUL); buf may be NULL. */
int sk_tunables(char *buf, int cap);

/* ---- instrumentation -------------------------------------------------- */
/* HIP-event durations (ms) of the kernels of the most recent *_dev / batch
 * call on this thread's device: prep (filter+stats), main (DTW or segment walk).
 * sk_detect_events_dev_i16 and sk_evs_push_dev_i16 are timed calls too: prep 0, main = all their launches (until the
 * event sessions came, a detect call left the figures of the timed call before it). */
int sk_last_kernel_ms(float *prep_ms, float *main_ms);
/* Reads of the most recent DTW call whose optimal path was longer than the two-pass
 * look-back window and were therefore recomputed by the exact single pass (diagnostic). */
int sk_last_dtw_retries(void);
/* Reads of the most recent DTW call whose path crossed the window pass's first (short) look-back and were redone
 * by its second tier (diagnostic; 0 when the call did not use the screening scheme). */
int sk_last_dtw_tier2(void);
/* Run-time guard of the screening scheme (the default DTW path: fixed-point screening + certified exact window).
 * Its exactness rests on a premise -- every screening cost lies within E = N + n + 2 units of the exact one -- that
 * is derived, not observed; the guard observes it.  out[0] results the window pass refused because the exact distance
 * contradicted the screening values (premise violations), out[1] reads the audit re-ran with the exact single pass
 * (one in 4 096, hashed; a call of few, long reads -- whose window passes are shorter than that one sweep -- is
 * audited one call in K <= 64, so that waiting for the sweep costs about 2 % on average: out[1] = 0 on the others;
 * SK_TUNING=1 SK_DTW_AUDIT_PERIOD=n audits every call), out[2] audited reads whose record differed (the exact record wins), out[3] reads kept
 * away from the screening because their sample image cannot be bounded tightly enough (exact pass, by design),
 * out[4] = out[0] + out[2] (the alarm), out[5] = 1 when the alarm made the library redo reads with the exact single
 * pass -- every read of the launch set that raised it (one motif over one ingest sub-batch) and of every later launch
 * set of the same call; launch sets of a multi-motif / sub-batched call that finished earlier passed their own premise
 * test and audit and are kept, out[6] reads whose candidate columns fell into two clusters and took a second window instead of the
 * exact pass (diagnostic), out[7] reserved.  In a healthy build out[0] = out[2] = out[4] = out[5] = 0, always.  The
 * two short forms return out[0] / out[2] (or a negative status).  The reference has no counterpart: mlpy's one
 * exact pass (/root/reference/MotifSeq.py:437-439) is what every record must equal. */
int sk_last_dtw_guard(int32_t *out /* [8] */);
int sk_last_dtw_premise_violations(void);
int sk_last_dtw_audit_mismatches(void);
/* Steps of the exact window pass in the most recent DTW call: out[0] = steps its wavefronts ran (the read groups of a
 * wavefront step together), out[1] = steps the reads asked for, summed over the groups.  bench.py prices the pass's own
 * issue roof with these (8 instructions per cell and step; mlpy's exact recurrence with start tracking,
 * /root/reference/MotifSeq.py:437-439).  Zeros when the call did not take the screening scheme. */
int sk_last_dtw_window_steps(uint64_t *out /* [2] */);
/* Reads of the most recent float64 call (sk_segment_*_f64, sk_motifseq_*_f64 with medmad) whose comparisons /
 * selection the streaming statistics kernel could not certify and that were redone in numpy's order (diagnostic);
 * -1 when the call did not use the streaming kernel (reads longer than 4 096 samples, zscale), or when a MotifSeq /
 * segmenter call of another route came after it. */
int sk_last_f64_retries(void);
/* Shader clock (GHz) the screening pass of the most recent DTW call ran at: its first wavefront counts shader cycles
 * (s_memtime) against the constant 100 MHz reference (s_memrealtime) over its whole sweep.  0 when the call did not
 * use the screening scheme.  bench.py prices the VALU-issue roofline at this clock instead of a nominal one. */
int sk_last_dtw_clock(double *ghz);
/* Per-launch view of the most recent two-pass DTW call: summed HIP-event time and launch count
 * of the distance pass (k_sdtw<..,DIST>) and of the start pass (k_sdtw<..,START>), and the reads
 * covered by the largest launch.  *dist_launches == 0 means the call used the single pass. */
int sk_last_dtw_profile(float *dist_ms, int *dist_launches, float *start_ms, int *start_launches,
                        int *reads_per_launch);
/* Synthetic squiggle generator on the device (bench input; not a reference
 * function): fills d_sig[nreads][nsamples] int16 deterministically from seed. */
int sk_synth_squiggles_dev(int16_t *d_sig, int64_t stride, int32_t nreads, int32_t nsamples,
                           uint64_t seed, const double *motif, int32_t nmotif);
/* Variants of the generator for bench.py's sensitivity runs and its multi-rank parity check (not reference
 * functions either).  Row r of a call is row row0 + r of the seed's batch, so any slice of any rank's batch can be
 * regenerated anywhere.  Defaults {0, 500, 0, 1, NULL, 0, 0} reproduce sk_synth_squiggles_dev. */
typedef struct sk_synth_opts {
    int64_t        row0;             /* first row of the seed's batch this call generates                      */
    int32_t        hit_permille;     /* reads carrying an exact copy of the motif (default 500)                */
    int32_t        stretch_permille; /* reads carrying the motif with every point repeated `stretch` times     */
    int32_t        stretch;          /* (their optimal path is that much wider: they take the exact retry)     */
    const int16_t *tmpl;             /* HOST pointer or NULL.  Non-NULL: every read is a window of this        */
    int32_t        ntmpl;            /* measured squiggle (ntmpl samples) at a random offset, plus rounded     */
    double         tmpl_noise;       /* N(0, tmpl_noise) noise; no plateaus / implants / spikes               */
} sk_synth_opts;
int sk_synth_variant_dev(int16_t *d_sig, int64_t stride, int32_t nreads, int32_t nsamples, uint64_t seed,
                         const double *motif, int32_t nmotif, const sk_synth_opts *o);
/* The float64 pA image of a device-resident int16 batch, value for value what SquigglePull writes for it
 * (SquigglePull.py:183-189,238-240: np.round((raw + offset) * range / digitisation, 2)) -- input for the float64
 * entry points (bench / tests; not a reference function of the hot path).  d_out: nreads * nsamples doubles,
 * d_off: nreads + 1 zero-based offsets (read r at r * nsamples). */
int sk_synth_pa_dev(const int16_t *d_raw, int64_t stride, int32_t nreads, int32_t nsamples,
                    double offset, double range, double digitisation, double *d_out, int64_t *d_off);

/* ---- SquigglePull text (SquigglePull.py) ------------------------------- */
/* Replaces, per read, SquigglePull's sample loop (SquigglePull.py:178-179, 211-212), its pA conversion
 * (convert_to_pA_numpy + np.round(.., 2), :185-189, 218-222, 238-240) and print_data (:243-253): the lines
 *     prefix[r] + tok(s0) + '\t' + ... + tok(s_{n-1}) + '\n'          (an empty read: prefix[r] + '\n')
 * in read order, made on the device.  prefix[r] = prefix[prefix_off[r] .. prefix_off[r+1]) is everything before the
 * first sample, trailing tab included (file name, read id, the -i columns), built by the caller.
 *   SK_PULL_RAW : tok = str(int(sample))
 *   SK_PULL_PA  : tok = str(np.round((sample + offset) * raw_unit, 2)) byte for byte: the integer
 *                 k = rint(((sample + offset) * raw_unit) * 100) printed with two decimals, a trailing zero dropped,
 *                 "-0.0" for a negative zero; raw_unit = float("%.2f" % range) / digitisation.
 * The host form takes calib[3 r ..] = digitisation, offset, range (what a fast5 / BLOW5 record carries; NULL in raw
 * mode), rows of `stride` samples with len[r] in [0, stride], and writes the text to `text` (capacity bytes) and
 * nreads + 1 line offsets to line_off (may be NULL; line_off[nreads] = *total).  *total always gets the text's size:
 * SK_ERR_OVERFLOW when it exceeds `capacity`, and then nothing is written to `text`.  SK_ERR_UNSUPPORTED: some pA
 * value is not finite or has |k| >= 1e15 (numpy would print it in another notation).
 * The _dev form: device pointers but `total` (host); d_cal2 = {offset, raw_unit} per read as sk_pa_calib makes them
 * (NULL in raw mode), d_line_off: nreads + 1 entries; len[r] is clamped into [0, stride]. */
typedef enum sk_pull_mode { SK_PULL_RAW = 0, SK_PULL_PA = 1 } sk_pull_mode;
int sk_pull_text(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const double *calib, int32_t mode,
                 const char *prefix, const int64_t *prefix_off, char *text, int64_t capacity, int64_t *total,
                 int64_t *line_off);
int sk_pull_text_dev(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, const double *d_cal2,
                     int32_t mode, const char *d_prefix, const int64_t *d_prefix_off, char *d_text, int64_t capacity,
                     int64_t *total, int64_t *d_line_off);

/* ---- event detection ---------------------------------------------------- */
/* A read cut into its own sequence of levels, without a model: a boundary wherever the current steps.  The definition is
 * the project's own ("Event detection"; tests/detect_ref.py states it in numpy); the reference has no such
 * step (its segmenter.py lists "push algorithm into C" and "integration with MotifSeq" as open).  Per read x[0..n) of raw
 * int16 samples -- no outlier filter, no [:Num] cut, raw coordinates throughout -- and per window w in (w_short, w_long),
 * with s1, s2 the sums and q1, q2 the sums of squares of x[i-w..i) and x[i..i+w), all exact integers:
 *     t_w[i] = sqrt( (double)((s2-s1)^2 * w) / (double)max(w*(q1+q2) - s1^2 - s2^2, 1) )   for w <= i <= n - w, else 0.0
 * (one correctly rounded division, one correctly rounded square root: the two-sample t-statistic, invariant under the
 * affine pA calibration).  Two peak detectors, short first, walk i = 0 .. n-1 with state pos = -1, val = +inf,
 * valid = false, masked_to = -1 each and cur = t_k[i]:
 *     skip the detector when i <= masked_to[k];
 *     pos == -1:  cur < val: val = cur;  else cur - val > peak_height: val = cur, pos = i;
 *     else:       cur > val: val = cur, pos = i;
 *                 k short and val > th_short: masked_to[long] = pos + w_short, the long detector back to its first state;
 *                 val - cur > peak_height and val > th_k: valid = true;
 *                 valid and i - pos > w_k / 2 (integer division): pos is marked; pos = -1, val = cur, valid = false.
 * Boundaries: 0, the marked positions (> 0, sorted, merged), n.  Events: the intervals between consecutive boundaries;
 * n = 0 has none, a read without a mark has [0, n).  A record holds an event's exact integers; mean = sum / length and
 * stdv = sqrt(max(length * sumsq - sum^2, 0)) / length are the host's to derive.
 * Valid parameters: 1 <= w_short <= w_long <= 64, finite thresholds, finite peak_height >= 0 (SK_ERR_INVALID otherwise).
 * Presets: dna = {3, 6, 1.4, 9.0, 0.2}, rna = {7, 14, 2.5, 9.0, 1.0}. */
typedef struct sk_det_params {      /* 32 bytes */
    int32_t w_short, w_long;
    double  th_short, th_long, peak_height;
} sk_det_params;
typedef struct sk_det_event {       /* 24 bytes */
    int32_t start, length;
    int64_t sum, sumsq;
} sk_det_event;
/* Rows of `stride` samples, len[r] clamped into [0, stride].  off gets nreads + 1 entries, always: read r's events are
 * rec[off[r] .. off[r+1]).  The records are written only when off[nreads] <= cap; otherwise the call returns
 * SK_ERR_OVERFLOW, off is complete and nothing is written to rec.  rec == NULL with cap == 0 is the counting call (it
 * returns SK_OK when there are no events at all).  NULL p / off, rec == NULL with cap > 0, cap < 0: SK_ERR_INVALID; the
 * arguments are checked before the device is looked at. */
int sk_detect_events_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                         const sk_det_params *p, int64_t *off /* [nreads + 1] */, sk_det_event *rec, int64_t cap);
/* device-resident form (all pointers device but p; nothing is synchronised): the check against cap happens on the
 * device, so the call returns SK_OK and the caller reads d_off[nreads] -- above cap, d_rec is untouched. */
int sk_detect_events_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                             const sk_det_params *p, int64_t *d_off /* [nreads + 1] */, sk_det_event *d_rec, int64_t cap);

/* ---- signal HMM: Viterbi per read ---------------------------------------- */
/* Every sample of a read assigned to one of up to SK_HMM_STATES named stretches (for a direct-RNA read: open pore,
 * leader, adapter, poly(A), transcript body) by the best path through a small hidden Markov model.  The definition is
 * the project's own ("Signal HMM"; tests/hmm_ref.py states it in numpy); the reference has no such step.
 * Everything is float64 add, subtract, multiply and the comparison `>`, one correctly rounded operation each (no
 * multiply-add, no log, no exp: the logarithms are taken when the model is built, on the host).
 *
 * Model (S = nstates, 1 <= S <= 6; rows and columns at and above S are ignored):
 *     linit[j], ltrans[i][j]   finite or -inf; at least one linit[j] finite
 *     c[j][m], mu[j][m], h[j][m], m = 0, 1: the two emission components of state j -- c finite or -inf (at least one
 *                              finite per state), mu finite, h finite and >= 0.  A Gaussian (weight, mean, sigma):
 *                              c = log(weight) - log(sigma * sqrt(2 pi)), h = 1 / (2 sigma^2); a flat component over
 *                              `range`: c = log(weight / range), h = 0; an absent component: c = -inf.
 * Samples: x_t = (double)raw_t, or with a calibration x_t = ((double)raw_t + offset_r) * unit_r -- the {offset, unit}
 * pair of read r as sk_pa_calib makes it and sk_pull_text_dev takes it, and no rounding to decimals.  limit > 0: only
 * the first min(len, limit) samples of a read are used (n below); never more than 0x7fffff00 of them.
 * Emission, with max(a, b) = (b > a ? b : a) throughout:
 *     a_m  = c[j][m] - ((x - mu[j][m]) * (x - mu[j][m])) * h[j][m]
 *     e_j(x) = max(a_0, a_1)
 * Recurrence:
 *     v_j(0) = linit[j] + e_j(x_0)
 *     v_j(t) = b_j + e_j(x_t),   b_j = max over i = 0 .. S-1, in rising i, of v_i(t-1) + ltrans[i][j]
 * -- a later i replaces an earlier one only when it is strictly greater: the lowest i wins ties, also ties at -inf.
 * No +inf can arise from valid input, so no NaN can (given |x - mu| < 2^511: the square stays finite).
 * Path summary instead of a back-trace: state j carries enter_j[0..6), enter_j[k] = the first sample at which the best
 * path into j was in state k, or -1.  t = 0: enter_j[j] = 0, the rest -1.  t >= 1: enter_j = the tuple of the winning
 * predecessor at t - 1, then enter_j[j] = t if it is still -1.
 * Result: f = the lowest j with the largest v_j(n - 1); score = v_f(n - 1), final_state = f, n_used = n,
 * enter = enter_f (-1 for k >= S).  n = 0: score 0.0, final_state -1, every enter -1. */
#define SK_HMM_STATES 6
typedef struct sk_hmm_model {       /* 632 bytes */
    int32_t nstates, reserved;
    double  linit[SK_HMM_STATES];
    double  ltrans[SK_HMM_STATES][SK_HMM_STATES];   /* [from][to] */
    double  c[SK_HMM_STATES][2], mu[SK_HMM_STATES][2], h[SK_HMM_STATES][2];
} sk_hmm_model;
typedef struct sk_hmm_rec {         /* 40 bytes */
    double  score;
    int32_t final_state, n_used;
    int32_t enter[SK_HMM_STATES];
} sk_hmm_rec;
/* Rows of `stride` int16 samples, len[r] in [0, stride]; cal2: NULL, or nreads {offset, unit} pairs; rec: nreads
 * records.  A model outside the rules above, NULL model / rec, limit < 0: SK_ERR_INVALID -- the arguments are checked
 * before the device is looked at. */
int sk_hmm_viterbi_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const double *cal2,
                       const sk_hmm_model *model, int32_t limit, sk_hmm_rec *rec);
/* device-resident form: every pointer is a device pointer but `model` (host); d_len[r] is clamped into [0, stride];
 * nothing is synchronised. */
int sk_hmm_viterbi_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, const double *d_cal2,
                           const sk_hmm_model *model, int32_t limit, sk_hmm_rec *d_rec);
/* ragged float64 values (pA, as a SquigglePull TSV holds them): read r = values[off[r] .. off[r+1]), x_t = the value. */
int sk_hmm_viterbi_f64_len(const double *values, const int64_t *off, int32_t nreads, const sk_hmm_model *model,
                           int32_t limit, sk_hmm_rec *rec);

/* ---- signal HMM: state paths --------------------------------------------- */
/* The best path itself, as run-length segments with exact statistics ("Signal HMM state paths";
 * tests/hmm_path_ref.py states it in numpy).  Model, samples, emission, recurrence and tie rules are those of the section
 * above, unchanged, and so is the sk_hmm_rec of every read.
 * Back pointer: for t >= 1 and j < S, arg_j(t) = the predecessor i that won b_j at t -- the lowest i wins ties, also ties
 *     at -inf.
 * Path: s(n - 1) = f, the record's final_state; s(t - 1) = arg_{s(t)}(t).
 * Segments: the maximal runs of equal s(t), in rising start; a read with n = 0 has none.
 * Winning component of sample t: m = 1 when a_1 > a_0 for state s(t), else m = 0 -- a_0, a_1 by e_j(x)'s operations in
 *     e_j(x)'s order, on the calibrated x where a calibration is given.
 * Record: n1 = the segment's samples whose component 1 won; sum[m] = the sum of the samples component m won, sumsq[m] the
 *     sum of their squares.  int16 rows: exact integers of the RAW samples, with or without cal2 (the calibration is
 *     affine: the host converts).  float64 values: doubles, each accumulated one sample at a time in rising t from 0.0 as
 *     sum += x and sumsq += x * x, every step one correctly rounded operation.
 * It follows that a read's segments tile [0, n), that neighbours differ in state, that the first start of state k is
 * enter[k], that the last segment's state is final_state, and that every step between neighbours has a finite ltrans. */
typedef struct sk_hmm_seg {         /* 48 bytes */
    int32_t state, start, length, n1;
    int64_t sum[2], sumsq[2];
} sk_hmm_seg;
typedef struct sk_hmm_segf {        /* 48 bytes: the float64 feed's record */
    int32_t state, start, length, n1;
    double  sum[2], sumsq[2];
} sk_hmm_segf;
/* The arguments of the matching sk_hmm_viterbi_* call, then off, seg and cap with sk_detect_events_*'s contract: off gets
 * nreads + 1 entries, always -- read r's segments are seg[off[r] .. off[r+1]).  The segments are written only when
 * off[nreads] <= cap; otherwise the call returns SK_ERR_OVERFLOW, rec and off are complete and nothing is written to seg.
 * seg == NULL with cap == 0 is the counting call (SK_OK when there is no segment at all).  Besides the checks of
 * sk_hmm_viterbi_*: NULL off, seg == NULL with cap > 0, cap < 0 are SK_ERR_INVALID, before the device is looked at. */
int sk_hmm_segments_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const double *cal2,
                        const sk_hmm_model *model, int32_t limit, sk_hmm_rec *rec, int64_t *off /* [nreads + 1] */,
                        sk_hmm_seg *seg, int64_t cap);
/* device-resident form (every pointer a device pointer but `model`; nothing is synchronised): returns SK_OK, the caller
 * reads d_off[nreads]; above cap the contents of d_seg are unspecified (nothing is written past d_seg[cap - 1]).  A
 * large batch is worked through in slices of whole 64-read groups, 4 bytes of scratch per sample padded to `stride` (or
 * `limit`) within a fixed budget. */
int sk_hmm_segments_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, const double *d_cal2,
                            const sk_hmm_model *model, int32_t limit, sk_hmm_rec *d_rec, int64_t *d_off /* [nreads + 1] */,
                            sk_hmm_seg *d_seg, int64_t cap);
int sk_hmm_segments_f64_len(const double *values, const int64_t *in_off, int32_t nreads, const sk_hmm_model *model,
                            int32_t limit, sk_hmm_rec *rec, int64_t *off /* [nreads + 1] */, sk_hmm_segf *seg, int64_t cap);

/* ---- signal HMM: posteriors ---------------------------------------------- */
/* How much probability stands behind a boundary: forward-backward over the model of the "signal HMM" section, the
 * expected counts of Baum-Welch, and optionally the posterior of every sample ("Signal HMM posteriors";
 * tests/hmm_post_ref.py states it in numpy).  Model, samples, calibration, limit and the emission e_j(x) = max(a_0, a_1)
 * are those of the "signal HMM" section, unchanged.  Every operation below is one correctly rounded float64 operation, in
 * the order written (no multiply-add).  Constants are given by their bit patterns.
 *
 * sk_exp(d):  if not d >= -700.0 (this covers -inf): 0.0.  Otherwise
 *     k = rint(d * LOG2E)                      round half to even
 *     r = (d - k * LN2_HI) - k * LN2_LO
 *     p = C13, then p = p * r + Cq for q = 12 .. 0
 *     result = ldexp(p, (int)k)                never subnormal: 2^-1010 is normal
 *     LOG2E = 0x3FF71547652B82FE, LN2_HI = 0x3FE62E42FEE00000, LN2_LO = 0x3DEA39EF35793C76; Cq = the double nearest 1 / q!:
 *     C0 = C1 = 0x3FF0000000000000, C2 = 0x3FE0000000000000, C3 = 0x3FC5555555555555, C4 = 0x3FA5555555555555,
 *     C5 = 0x3F81111111111111, C6 = 0x3F56C16C16C16C17, C7 = 0x3F2A01A01A01A01A, C8 = 0x3EFA01A01A01A01A,
 *     C9 = 0x3EC71DE3A556C734, C10 = 0x3E927E4FB7789F5C, C11 = 0x3E5AE64567F544E4, C12 = 0x3E21EED8EFF8D898,
 *     C13 = 0x3DE6124613A86D09.
 * sk_log(s), 1 <= s < 8:  f = s, k = 0; three times: if f > SQRT2 then f = f * 0.5, k = k + 1;
 *     z = (f - 1.0) / (f + 1.0) -- the IEEE division --, z2 = z * z
 *     p = D23, then p = p * z2 + Dq for q = 21, 19, .., 1
 *     result = k * LN2 + (z + z) * p
 *     SQRT2 = 0x3FF6A09E667F3BCD, LN2 = 0x3FE62E42FEFA39EF; Dq = the double nearest 1 / q: D1 = 0x3FF0000000000000,
 *     D3 = 0x3FD5555555555555, D5 = 0x3FC999999999999A, D7 = 0x3FC2492492492492, D9 = 0x3FBC71C71C71C71C,
 *     D11 = 0x3FB745D1745D1746, D13 = 0x3FB3B13B13B13B14, D15 = 0x3FB1111111111111, D17 = 0x3FAE1E1E1E1E1E1E,
 *     D19 = 0x3FAAF286BCA1AF28, D21 = 0x3FA8618618618618, D23 = 0x3FA642C8590B2164.
 * lse(c_0 .. c_{K-1}):  m = the maximum in rising index, by `>`; if m == -inf the result is -inf; otherwise s = 0.0, then
 *     s = s + sk_exp(c_i - m) in rising i; the result is m + sk_log(s) (1 <= s <= K <= 6).  A candidate of -inf adds an
 *     exact 0.0.
 * Forward:    alpha_j(0) = linit[j] + e_j(x_0);  alpha_j(t) = lse_i(alpha_i(t-1) + ltrans[i][j]) + e_j(x_t);
 *             L = lse_j alpha_j(n-1).
 * Backward:   beta_i(n-1) = 0.0;  u_ij(t) = ltrans[i][j] + (e_j(x_{t+1}) + beta_j(t+1));  beta_i(t) = lse_j u_ij(t).
 * Posteriors: gamma_j(t) = sk_exp((alpha_j(t) + beta_j(t)) - L);
 *             xi_ij(t) = sk_exp((alpha_i(t) + u_ij(t)) - L) for t <= n - 2.
 * Record sk_hmm_post: loglik = L, n_used = n, final_post[j] = gamma_j(n-1); occ[j] starts at 0.0 and takes
 *     occ[j] += gamma_j(t) for t = n-1 down to 0.  Entries at and above S are 0.0.
 * Record sk_hmm_counts (optional): for falling t, with m the winning component of state j at x_t (m = 1 when a_1 > a_0),
 *     n[j][m] += gamma, sx[j][m] += gamma * x, sxx[j][m] += gamma * (x * x), x in model units (after any calibration);
 *     xi[i][j] += xi_ij(t) for t = n-2 down to 0; init[j] = gamma_j(0).  Every sum starts at 0.0.
 * Dense posteriors (optional): the caller gives goff [nreads + 1], the running sum of n_used from goff[0] = 0 (it knows n
 *     from len and limit); gamma[(goff[r] + t) * 6 + j] = gamma_j(t), 0.0 for j >= S.
 * n = 0: loglik 0.0, flags 0, everything else 0.  L == -inf (a model with a dead end): loglik -inf, flags =
 *     SK_HMM_POST_IMPOSSIBLE, every probability and count 0.0, dense rows included.
 * No NaN is ever written: valid input gives no +inf (as in the "signal HMM" section), so alpha, beta and L are finite or
 *     -inf; lse answers -inf before it would form -inf - -inf; sk_exp is given a finite number or -inf and answers the
 *     latter with 0.0; and a read with L == -inf is answered with zeros instead of sk_exp(.. - L). */
#define SK_HMM_POST_IMPOSSIBLE 1
typedef struct sk_hmm_post {        /* 112 bytes */
    double  loglik;
    int32_t n_used, flags;
    double  final_post[SK_HMM_STATES];
    double  occ[SK_HMM_STATES];
} sk_hmm_post;
typedef struct sk_hmm_counts {      /* 624 bytes */
    double  n[SK_HMM_STATES][2], sx[SK_HMM_STATES][2], sxx[SK_HMM_STATES][2];
    double  xi[SK_HMM_STATES][SK_HMM_STATES];       /* [from][to] */
    double  init[SK_HMM_STATES];
} sk_hmm_counts;
/* The arguments of sk_hmm_viterbi_i16 with post [nreads] in rec's place, then counts [nreads] or NULL, then goff
 * [nreads + 1] and gamma [goff[nreads] * 6] or both NULL.  The checks are sk_hmm_viterbi_*'s; in addition exactly one of
 * goff / gamma being NULL is SK_ERR_INVALID -- all before the device is looked at.  The host forms also refuse a goff
 * that is not the running sum of n_used. */
int sk_hmm_posterior_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const double *cal2,
                         const sk_hmm_model *model, int32_t limit, sk_hmm_post *post, sk_hmm_counts *counts,
                         const int64_t *goff, double *gamma);
/* device-resident form: every pointer is a device pointer but `model` (host); d_len[r] is clamped into [0, stride];
 * nothing is synchronised.  d_goff is the caller's promise: rows [d_goff[r], d_goff[r] + n_used) of d_gamma are written.
 * Scratch: 3 072 bytes per 64 reads and 128 samples, and 393 216 bytes per 64 reads of a slice; a large batch is worked
 * through in slices of whole 64-read groups within a fixed budget. */
int sk_hmm_posterior_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                             const double *d_cal2, const sk_hmm_model *model, int32_t limit, sk_hmm_post *d_post,
                             sk_hmm_counts *d_counts, const int64_t *d_goff, double *d_gamma);
/* ragged float64 values: read r = values[off[r] .. off[r+1]), x_t = the value. */
int sk_hmm_posterior_f64_len(const double *values, const int64_t *off, int32_t nreads, const sk_hmm_model *model,
                             int32_t limit, sk_hmm_post *post, sk_hmm_counts *counts, const int64_t *goff, double *gamma);

/* ---- MotifSeq sessions: search reads chunk by chunk as they arrive --------- */
/* A session owns K motifs (at most 1 024 points each), nslots slots -- one read in progress each, e.g. one per sequencer
 * channel --, the filter limits, a scale mode and a calibration length W = calib ("MotifSeq sessions";
 * tests/stream_ref.py states the definition in numpy).  Let raw be all samples pushed to a slot since its last reset,
 * kept = raw after the filter (scale_low < x < scale_hi, raw units), n = len(kept), seen = len(raw).
 * Calibration: while n < W and the slot has not been flushed it is calibrating: it buffers its kept samples and its
 *     records are dist = tail = NaN, start = end = -1, n, seen, flags = SK_FLAG_CALIBRATING.  When n reaches W, center
 *     and scale are fixed from the first W kept samples (a flush with n >= 1: from all n) -- exactly the statistics
 *     sk_motifseq_multi_batch_i16 takes of that row -- and never change afterwards.  A reset may hand the slot a
 *     (center, scale) pair instead; that slot never calibrates.
 * Search: with y = ((double)kept - center) / scale the record of motif k after any push is that of
 *     dtw_subsequence(motif_k, y): dist = the first minimum of cost[-1, :], end its column, start by the back-trace
 *     (diagonal, then j - 1, then i - 1), tail = cost[-1, n - 1]: the cost of the best match that ends at the newest
 *     sample.  start, end and n are in kept coordinates.  n = 0: dist = tail = NaN, start = end = -1.
 * medmad with MAD 0: SK_FLAG_DEGENERATE, NaN distances and -1 coordinates until the slot is reset.  A flush at n = 0:
 *     SK_FLAG_EMPTY (a calibrating slot then stays without statistics, NaN / -1, until it is reset).
 * The record depends only on the samples pushed so far -- not on how they were cut into chunks, which other slots
 * shared the call, or the slot's number; a read of n <= W samples pushed in any chunks and flushed has the dist, start,
 * end, n and flags of sk_motifseq_multi_batch_i16 on the whole read -- field for field, so a slot whose calibration a
 * flush ended on a MAD of 0 reports the dist = +inf that call leaves for such a read (tail stays NaN), not NaN.
 * chunks counts the pushes of len > 0 the read has had; a push of len 0 is a peek and changes nothing. */
#define SK_STREAM_MAX_CALIB 65536
#define SK_STREAM_MAX_SESSIONS 8
enum { SK_FLAG_CALIBRATING = 8 };  /* sk_stream_rec.flags: the slot still collects its calibration samples */
typedef struct sk_stream_params {   /* 32 bytes */
    int32_t scale_mode;             /* SK_SCALE_MEDMAD or SK_SCALE_ZSCALE */
    int32_t scale_low, scale_hi;
    int32_t calib;                  /* W: 1 .. SK_STREAM_MAX_CALIB */
    int32_t nslots;                 /* 1 .. 65536 */
    int32_t reserved[3];            /* 0 */
} sk_stream_params;
typedef struct sk_stream_rec {      /* 40 bytes */
    double  dist, tail;
    int32_t start, end, n, seen, flags, chunks;
} sk_stream_rec;
/* motif k = motifs[motif_off[k] .. motif_off[k + 1]).  The session belongs to the context the calling thread is bound
 * to (at most SK_STREAM_MAX_SESSIONS per context; the handle is valid for threads bound to it; sk_shutdown closes them).
 * SK_ERR_INVALID: no motifs, an empty motif, calib or nslots out of range, non-zero reserved words, an unknown scale
 * mode; SK_ERR_UNSUPPORTED: a motif of more than 1 024 points. */
int sk_stream_open(const double *motifs, const int32_t *motif_off, int32_t nmotifs, const sk_stream_params *p,
                   int32_t *handle);
/* Appends len[i] samples (row i of `rows`, `stride` apart; 0 <= len[i] <= stride) to slot slots[i], i < m, and returns
 * every named slot's records, out [nmotifs][m].  A slot may appear once per call (host form: SK_ERR_INVALID otherwise,
 * like a slot out of range or an unknown handle). */
int sk_stream_push_i16(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride,
                       const int32_t *len, sk_stream_rec *out);
/* device-resident form: every pointer is a device pointer, nothing is synchronised; distinct slots are the caller's
 * contract, d_len[i] is clamped into [0, stride] and an entry whose slot is out of range is skipped (its records: NaN,
 * -1 and zero counts). */
int sk_stream_push_dev_i16(int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows, int64_t stride,
                           const int32_t *d_len, sk_stream_rec *d_out);
/* Ends the calibration of the named slots with what they hold (see above) and returns their records like a push. */
int sk_stream_flush(int32_t handle, const int32_t *slots, int32_t m, sk_stream_rec *out);
/* Starts a new read in the named slots.  center and scale both NULL: the slots calibrate; both given ([m], scale finite
 * and not 0, center finite): they search under that normalisation from their first sample. */
int sk_stream_reset(int32_t handle, const int32_t *slots, int32_t m, const double *center, const double *scale);
int sk_stream_close(int32_t handle);

/* ---- Mapping sessions: the pair-list DTW continued as a read's points arrive ----------------------------------------
 * sk_dtw_pairs searches finished queries of at most 1 024 points.  A mapping session keeps `nslots` queries in
 * progress (a channel's event levels, say) and searches each of them in every one of `ntargets` targets as the points
 * arrive: a push appends a chunk of points to each named slot and returns, per target, the record of everything the
 * slot has been given since its reset.  Per (slot, target) the session keeps the LAST ROW of the DTW matrix, D (float64)
 * and the back-trace start S (int32) per target column; a push sweeps only the new rows.
 * Targets: copied to the device at open; target t = targets[target_off[t] .. target_off[t + 1]), at least one point
 *     each (SK_ERR_INVALID for an empty one, naming it).
 * Row state: nslots * (sum of the target lengths) * 12 bytes, updated in place.  SK_ERR_UNSUPPORTED, with the bytes in
 *     the message, when that exceeds SK_MAP_MAX_STATE_BYTES.
 * A push: chunk i = values[off[i] .. off[i + 1]) -- float64 points, normalised by the caller -- is appended to slot
 *     slots[i], i < m.  A chunk of length 0 is a peek: it changes nothing and returns the slot's last records.  A slot
 *     may appear once per push; a chunk holds at most SK_MAP_MAX_CHUNK points (longer ones are the caller's to cut);
 *     slots not named are untouched.  A chunk of more than 1 024 points is swept in pieces of 1 024 rows.
 * The record after a push: out[t * m + i].(dist, start, end, n, flags) is sk_dtw_subsequence(all points slot slots[i]
 *     has been given since its reset, target t), bit for bit -- whatever the cuts, whichever slots shared the push and
 *     whatever the total (no limit of 1 024 points: every cell is one correctly rounded add of correctly rounded operands
 *     and the tie order of the start propagation is a per-cell rule, so rows continued from the stored row are the rows
 *     of the one-shot sweep).  n is the target's length.  rows = the points given since the reset, pushes = the pushes
 *     of length > 0 since the reset.  A slot without points: dist NaN, start = end = -1, rows = pushes = 0.
 * Limits: SK_MAP_MAX_SESSIONS sessions per context, 1 .. SK_MAP_MAX_SLOTS slots, 1 .. SK_MAP_MAX_TARGETS targets,
 *     nslots * ntargets <= 2^30.  sk_shutdown closes open sessions.
 * Refusals (SK_ERR_INVALID unless said otherwise) name the entry, slot or target.  Those the arguments alone decide
 *     come before any device work, in this order: a handle outside [0, SK_MAP_MAX_SESSIONS), m < 0, NULL pointers,
 *     offsets that decrease, a chunk above SK_MAP_MAX_CHUNK (SK_ERR_UNSUPPORTED), (host form) a slot outside
 *     [0, SK_MAP_MAX_SLOTS), a slot twice.  Then the session: a handle that is not open, a slot outside [0, nslots).
 *     A refused push changes nothing. */
#define SK_MAP_MAX_SESSIONS 8
#define SK_MAP_MAX_SLOTS 65536
#define SK_MAP_MAX_TARGETS 65536
#define SK_MAP_MAX_CHUNK 65536
#define SK_MAP_MAX_STATE_BYTES ((int64_t)1 << 35)      /* 32 GiB */
typedef struct sk_map_rec {      /* 32 bytes */
    double  dist;
    int32_t start, end, n, flags;   /* sk_hit's fields: n = the target's length */
    int32_t rows;                /* query points this slot has been given since its reset */
    int32_t pushes;              /* pushes of length > 0 since its reset */
} sk_map_rec;
int sk_map_open(const double *targets, const int64_t *target_off, int32_t ntargets, int32_t nslots, int32_t *handle);
/* values, off, slots and out are host pointers; the records are complete when the call returns. */
int sk_map_push(int32_t handle, const int32_t *slots, int32_t m, const double *values, const int64_t *off,
                sk_map_rec *out);      /* out [ntargets][m] */
/* device-resident form: d_slots, d_values (chunk i at d_values[off[i] - off[0]]) and d_out are device pointers, off is a
 * host pointer (the plan is made from the chunk lengths).  The slot numbers are read back (one small copy) and checked
 * as in the host form; nothing is synchronised behind the launches. */
int sk_map_push_dev(int32_t handle, const int32_t *d_slots, int32_t m, const double *d_values, const int64_t *off,
                    sk_map_rec *d_out);
/* The named slots start a new query: rows = pushes = 0, their row state is ignored from then on. */
int sk_map_reset(int32_t handle, const int32_t *slots, int32_t m);
int sk_map_close(int32_t handle);
/* The last push of the calling thread's context: bytes of row state of its session, (piece, target) entries swept,
 * sweep launches (one per piece index and (L, R) group).  Any pointer may be NULL. */
int sk_last_map_plan(int64_t *state_bytes, int64_t *entries, int64_t *launches);

/* ---- Hit lists over a pair list: up to max_hits non-overlapping loci per pair and per session slot ------------------
 * sk_dtw_pairs and a mapping session's push report one locus per (query, target): the first argmin of the last row.
 * A hit list keeps going, by the rule of the MotifSeq hit lists above.  For a query x of N points and a target y of M
 * points let d_j = D[N-1][j] of sk_dtw_subsequence(x, y) and s_j the column where mlpy's back-trace from (N-1, j) ends
 * (tie order: diagonal, then left, then up).  max_hits rounds; each takes the smallest admissible d_j, ties to the
 * smallest j; a column is admissible if d_j <= max_dist and [s_j, j] is disjoint from every interval taken before.
 * Records: hit k of a list is an sk_hit (dist = d_j, start = s_j, end = j, n = M, flags); an unused slot holds dist NaN,
 *     start = end = -1 and the pair's n and flags; count is the number of hits.  An empty target: count 0, n = 0 and
 *     SK_FLAG_EMPTY in every slot.  With max_dist = +inf hit 1 is sk_dtw_pairs' record byte for byte.
 * Limits: max_hits 1 .. 64; max_dist not NaN (+inf: no cut); subsequence mode only; a query holds 1 .. 1 024 points.
 * sk_dtw_pairs_hits: the arguments, checks, codes and messages of sk_dtw_pairs (subsequence mode), then the two limits
 *     above, then NULL out / count -- all of it before a context is looked for; npairs = 0 is SK_OK.  The last rows
 *     (12 bytes per target column) are kept for a slice of the list at a time: slices of consecutive pairs whose rows fit
 *     the row buffer of the MotifSeq hit lists (2 GiB), at least one pair each.  out [npairs][max_hits], count [npairs].
 * sk_dtw_pairs_hits_dev: d_values, d_out and d_count are device pointers, off and pairs host pointers; nothing is
 *     synchronised behind the last launch.
 * sk_map_hits: the lists of the named slots of a mapping session against every target, selected from the rows the
 *     pushes stored: nothing is swept and nothing of the session changes.  out [ntargets][m][max_hits], count
 *     [ntargets][m].  Hit 1 equals the sk_hit fields of the slot's last push record.  A slot without points: count 0,
 *     every slot dist NaN, start = end = -1, n = the target's length, flags 0.  Slots are checked as sk_map_push checks
 *     them (refusals in its order, the two limits above after m < 0); a refused call writes nothing.
 * sk_map_hits_dev: d_slots, d_out and d_count are device pointers; the slot numbers are read back (one small copy).
 * sk_last_pair_hits_plan: the last of these calls on the calling thread's context -- bytes of last rows selected from at
 *     a time, slices (1 for a session), rows of more than 4 096 columns (those take a workgroup each, the others a
 *     wavefront each).  Any pointer may be NULL. */
int sk_dtw_pairs_hits(const double *values, const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs,
                      int32_t max_hits, double max_dist, sk_hit *out, int32_t *count);
int sk_dtw_pairs_hits_dev(const double *d_values, const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs,
                          int32_t max_hits, double max_dist, sk_hit *d_out, int32_t *d_count);
int sk_map_hits(int32_t handle, const int32_t *slots, int32_t m, int32_t max_hits, double max_dist, sk_hit *out,
                int32_t *count);
int sk_map_hits_dev(int32_t handle, const int32_t *d_slots, int32_t m, int32_t max_hits, double max_dist, sk_hit *d_out,
                    int32_t *d_count);
int sk_last_pair_hits_plan(int64_t *row_bytes, int64_t *slices, int64_t *long_rows);

/* ---- Event sessions: a read cut into events as its samples arrive ---------------------------------------------------
 * sk_detect_events_* takes whole reads.  An event session keeps `nslots` reads in progress under one sk_det_params and
 * cuts each of them as its samples arrive.  A slot holds n, the samples it has been given since its reset, the walk
 * position i, both detectors' states and the last boundary: O(1) state, 416 bytes per slot (160 of state, the last 128
 * samples), no sample of an event is kept however long the event.
 * A push: the first len[k] samples of row k (rows + k * stride, int16) are appended to slot slots[k], k < m; then the
 *     slot's positions i are walked while i + w_long <= n.  For those positions t_short[i] and t_long[i] are what they
 *     will be in the finished read, whatever follows.  Every mark closes the event [last boundary, pos) and emits its
 *     record at once, in read coordinates: the marks of both detectors together come in strictly rising order, so an
 *     event is final the moment its end is marked.
 * END: end[k] != 0 says the read ends with this chunk (which may be empty).  The remaining positions up to n - 1 are
 *     walked under the one-shot rule (t_w[i] = 0 for i > n - w, samples at and beyond n count as 0 in the window sums)
 *     and the closing event [last boundary, n) is emitted (none for n = 0).  An ended slot takes no samples until it is
 *     reset; an empty chunk for it, END or not, does nothing.  end == NULL: no entry ends.
 * The records: off gets m + 1 entries, always; entry k's new events are rec[off[k] .. off[k + 1]).  The concatenation of
 *     everything a slot has emitted from its reset to END is sk_detect_events_i16's array of all its samples, byte for
 *     byte, whatever the cuts (reads shorter than 2 w, of 1 or of 0 samples included); after any push it is a prefix of
 *     that array (tests/evstream_ref.py states which).
 * Overflow: when off[m] > cap the host form returns SK_ERR_OVERFLOW with off complete and rec untouched.  Nothing is
 *     lost: the session keeps the last push's records on the device until its next push, and sk_evs_fetch delivers them.
 * Limits: SK_EVS_MAX_SESSIONS sessions per context, 1 .. SK_EVS_MAX_SLOTS slots, a slot holds at most 2^31 - 1 samples,
 *     m * (stride + 64) at most 2^31 in a push (SK_ERR_UNSUPPORTED).  sk_shutdown closes open sessions.
 * Refusals (SK_ERR_INVALID unless said otherwise).  Those the arguments alone decide come before a context is looked
 *     for: a handle outside [0, SK_EVS_MAX_SESSIONS), m < 0, NULL pointers (end may be NULL; rec may be NULL with
 *     cap == 0), stride < 0, cap < 0, (host form) a negative len or one above stride, a slot outside
 *     [0, SK_EVS_MAX_SLOTS), a slot twice; at open NULL p / handle, parameters outside sk_detect_events' ranges, nslots
 *     outside 1 .. SK_EVS_MAX_SLOTS.  Then the session: a handle that is not open, a slot outside [0, nslots), samples
 *     for an ended slot, a slot whose total would pass 2^31 - 1 samples (SK_ERR_UNSUPPORTED).  A refused push changes
 *     nothing. */
#define SK_EVS_MAX_SESSIONS 8
#define SK_EVS_MAX_SLOTS 1048576
int sk_evs_open(const sk_det_params *p, int32_t nslots, int32_t *handle);
/* every pointer a host pointer; off and (when off[m] <= cap) rec are complete when the call returns. */
int sk_evs_push_i16(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride,
                    const int32_t *len, const int32_t *end /* may be NULL */, int64_t *off /* [m + 1] */,
                    sk_det_event *rec, int64_t cap);
/* device-resident form: every pointer a device pointer, nothing is synchronised.  Distinct slots inside [0, nslots) are
 * the caller's contract (an entry with a slot outside is ignored); len is clamped into [0, stride]; samples for an
 * ended slot are ignored.  The check against cap happens on the device, as in sk_detect_events_dev_i16: the call returns
 * SK_OK and the caller reads d_off[m] -- above cap, d_rec is untouched and sk_evs_fetch has the records. */
int sk_evs_push_dev_i16(int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows, int64_t stride,
                        const int32_t *d_len, const int32_t *d_end /* may be NULL */, int64_t *d_off /* [m + 1] */,
                        sk_det_event *d_rec, int64_t cap);
/* The records the session kept from its last push, compact and in that push's order, to rec (host).  SK_ERR_OVERFLOW
 * when they are more than cap (nothing written); no push yet: nothing to copy, SK_OK. */
int sk_evs_fetch(int32_t handle, sk_det_event *rec, int64_t cap);
/* The named slots start a new read: n = 0, both detectors in their first state, not ended. */
int sk_evs_reset(int32_t handle, const int32_t *slots, int32_t m);
int sk_evs_close(int32_t handle);
/* The last push of the calling thread's context: bytes of slot state of its session, staging rows it reserved
 * (m * rows per entry).  guard_hits: the slots that the pushes of ALL event sessions of the context have stopped at a
 * guard since the context was set up -- it only counts up, so one look after any number of pushes covers them all (a
 * lane that would overrun its staging rows, meet a mark at or below its last boundary or pass 2^31 - 1 samples: always
 * 0 unless the facts the staging rests on are wrong).  Reading it waits for the pushes.  Any pointer may be NULL. */
int sk_last_evs_plan(int64_t *state_bytes, int64_t *staged_records, int64_t *guard_hits);

/* ---- HMM sessions: Viterbi continued as a read's samples arrive -----------------------------------------------------
 * sk_hmm_viterbi_* takes finished reads.  An HMM session owns one sk_hmm_model -- checked by the rules of the "signal
 * HMM" section and copied at open -- and `nslots` slots, each a read in progress.  Viterbi carries O(1) state and never
 * looks ahead, so a slot holds just that state, 224 bytes: the six scores v (float64), the six enter tuples E[6][6]
 * (int32), n (the samples since its reset), pushes, and the slot's calibration pair {offset, unit} ({0.0, 1.0}: none).
 * The sample feed, emission, recurrence, tie order and enter rule are those of the "signal HMM" section, unchanged.  A
 *     push appends samples t = n, n + 1, .. to the slot: t == 0 takes the linit rule, t >= 1 the recurrence on the stored
 *     v and E; enter indices are in read coordinates.  Two feeds write to the same state:
 *       int16 rows with len    x = ((double)raw + offset) * unit with the slot's pair, as sk_hmm_viterbi_i16 does it;
 *       ragged float64 values  x = the value; chunk i = values[off[i] .. off[i + 1]) -- pA text, event levels.
 * The record after a push, one sk_hmms_rec (96 bytes) per entry: score, final_state, n_used, enter[6] are the 40 bytes of
 *     sk_hmm_rec, field for field, and equal sk_hmm_viterbi_* on all the samples the slot has had since its reset --
 *     whatever the cuts, whichever slots shared the push, whichever slot number the read has.  v[j] = v_j(n - 1) for
 *     j < S and -inf for j >= S.  At n == 0 every v is -inf and the first 40 bytes are the one-shot's empty record.
 *     pushes counts the pushes of length > 0; flags is 0 (reserved).
 * A chunk of length 0 is a peek: it returns the record and changes nothing.  There is no END flag: without look-ahead the
 *     record after the last push is the finished read's.
 * Limits: SK_HMMS_MAX_SESSIONS sessions per context, 1 .. SK_HMMS_MAX_SLOTS slots, a slot holds at most 0x7fffff00
 *     samples (the one-shot's cap), m * (stride + 64) at most 2^31 in an int16 push (SK_ERR_UNSUPPORTED).  sk_shutdown
 *     closes open sessions.
 * Refusals (SK_ERR_INVALID unless said otherwise).  Those the arguments alone decide come before a context is looked
 *     for: a handle outside [0, SK_HMMS_MAX_SESSIONS), m < 0, NULL pointers (with m > 0; in the host form values may be NULL
 *     when no chunk has a sample), stride < 0, (host forms) a negative len or one above stride, offsets that decrease, a slot outside
 *     [0, SK_HMMS_MAX_SLOTS), a slot twice; at open a model that breaks the rules (sk_hmm_viterbi's message), NULL
 *     handle, nslots outside 1 .. SK_HMMS_MAX_SLOTS; at reset a cal2 pair that is not finite.  Then the session: a handle
 *     that is not open, a slot outside [0, nslots), a slot whose total would pass the cap (SK_ERR_UNSUPPORTED).  A
 *     refused push changes nothing. */
#define SK_HMMS_MAX_SESSIONS 8
#define SK_HMMS_MAX_SLOTS 1048576
typedef struct sk_hmms_rec {        /* 96 bytes */
    double  score;                  /* the 40 bytes of sk_hmm_rec ... */
    int32_t final_state, n_used;
    int32_t enter[SK_HMM_STATES];
    double  v[SK_HMM_STATES];       /* v_j(n - 1); -inf for j >= S and at n == 0 */
    int32_t pushes, flags;
} sk_hmms_rec;
int sk_hmms_open(const sk_hmm_model *model, int32_t nslots, int32_t *handle);
/* every pointer a host pointer; the first len[k] samples of row k (rows + k * stride) go to slot slots[k]; out [m] is
 * complete when the call returns. */
int sk_hmms_push_i16(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride,
                     const int32_t *len, sk_hmms_rec *out);
/* device-resident form: every pointer a device pointer, nothing is synchronised.  Distinct slots inside [0, nslots) are
 * the caller's contract: an entry with a slot outside is skipped and its record is the empty record (n_used 0, every v
 * -inf, pushes 0).  len is clamped into [0, stride]; samples beyond a slot's cap are ignored and the slot is counted in
 * guard_hits. */
int sk_hmms_push_dev_i16(int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows, int64_t stride,
                         const int32_t *d_len, sk_hmms_rec *d_out);
/* ragged float64 values: chunk i = values[off[i] .. off[i + 1]), off [m + 1]; host pointers. */
int sk_hmms_push_f64(int32_t handle, const int32_t *slots, int32_t m, const double *values, const int64_t *off,
                     sk_hmms_rec *out);
/* ... d_slots, d_values, d_off [m + 1] and d_out all device pointers, as sk_hmms_push_dev_i16. */
int sk_hmms_push_dev_f64(int32_t handle, const int32_t *d_slots, int32_t m, const double *d_values, const int64_t *d_off,
                         sk_hmms_rec *d_out);
/* The named slots start a new read: n = pushes = 0, every v -inf.  cal2: NULL (no calibration: {0.0, 1.0}), or m
 * {offset, unit} pairs, the slots' from then on (the int16 feed uses them). */
int sk_hmms_reset(int32_t handle, const int32_t *slots, int32_t m, const double *cal2);
int sk_hmms_close(int32_t handle);
/* The last push of the calling thread's context: bytes of slot state of its session.  guard_hits: the entries of the
 * device-form pushes of ALL HMM sessions of the context that brought samples beyond their slot's cap since the context
 * was set up -- it only counts up, so one look after any number of pushes covers them all.  Reading it waits for the
 * pushes.  Either pointer may be NULL. */
int sk_last_hmms_plan(int64_t *state_bytes, int64_t *guard_hits);
/* Filtered sessions: the forward recursion of "signal HMM: posteriors" carried beside the Viterbi pass.
 * A session opened with SK_HMMS_FILTER keeps, beside each 224-byte slot, alpha[6] (float64, 48 bytes, an array of its
 *     own): the slot layout and a plain session's state_bytes = nslots * 224 stay as they are, a filtered session reports
 *     nslots * 272.  A reset sets every alpha to -inf.  A push appends samples t = n, n + 1, .. for either feed:
 *       t == 0   alpha_j = linit[j] + e_j(x) for j < S;
 *       t >= 1   alpha_j = lse_i(alpha_i + ltrans[i][j]) + e_j(x), with sk_exp, sk_log and lse exactly as that section
 *                states them (the forward step of sk_hmm_posterior_*, transitions of -inf skipped as there);
 *     x is the value the Viterbi step of the same sample sees, and samples past the slot's cap are ignored by both
 *     recurrences alike.  The Viterbi side of the slot and sk_hmms_rec are untouched: a filtered session's records are
 *     byte for byte a plain session's.
 * The filter of a slot, sk_hmms_filt (64 bytes).  n == 0: all zero.  Otherwise L = lse_j alpha_j in rising j < S,
 *     loglik = L, post[j] = sk_exp((alpha_j + 0.0) - L) for j < S and 0.0 above: P(state at the newest sample | the samples
 *     so far).  L == -inf: loglik = -inf, flags = SK_HMM_POST_IMPOSSIBLE, every post 0.0.  No NaN is ever written, by that
 *     section's argument.  For a read of n samples the one-shot record has beta(n - 1) = 0.0, so loglik and post are
 *     sk_hmm_posterior_*'s loglik and final_post of the samples the slot has had since its reset, bit for bit, whatever
 *     the cuts.
 * sk_hmms_open_ex: flags == 0 is sk_hmms_open exactly; the only other value is SK_HMMS_FILTER; unknown bits are
 *     SK_ERR_INVALID by the arguments alone, before sk_hmms_open's own refusals.  The four push entries and sk_hmms_reset
 *     take filtered handles as they are.
 * sk_hmms_filter (host pointers) reads the named slots as they stand and changes nothing; a slot may appear twice.
 *     sk_hmms_filter_dev: device pointers, stream-ordered, nothing synchronised; an entry whose slot lies outside
 *     [0, nslots) gets the all-zero record.
 * Refusals (SK_ERR_INVALID), in the section's order.  By the arguments alone: a handle outside the table, m < 0, a NULL
 *     pointer with m > 0, (host form) a slot outside [0, SK_HMMS_MAX_SLOTS).  Then by the session: a handle that is not
 *     open, (host form) a slot at or above nslots, a handle that was opened without SK_HMMS_FILTER (the message says so).
 *     A refused call leaves out untouched. */
#define SK_HMMS_FILTER 1
typedef struct sk_hmms_filt {       /* 64 bytes */
    double  loglik;                 /* log P(the samples so far); 0.0 at n == 0 */
    int32_t n_used, flags;          /* flags: SK_HMM_POST_IMPOSSIBLE */
    double  post[SK_HMM_STATES];    /* P(state j at sample n - 1 | samples 0 .. n - 1) */
} sk_hmms_filt;
int sk_hmms_open_ex(const sk_hmm_model *model, int32_t nslots, int32_t flags, int32_t *handle);
int sk_hmms_filter(int32_t handle, const int32_t *slots, int32_t m, sk_hmms_filt *out);
int sk_hmms_filter_dev(int32_t handle, const int32_t *d_slots, int32_t m, sk_hmms_filt *d_out);

/* ---- Live mapping sessions: samples in, mapping records and decisions out --------------------------------------------
 * An event session cuts events, a mapping session continues the DTW; what a selective-sequencing client needs between
 * them -- the level of every event, held back until the read can be normalised, then normalised -- and behind them -- one
 * decision per read -- is this section.  A live session keeps `nslots` channels in progress under one sk_det_params, one
 * calibration length C = calib and one set of targets.  It owns an event session and a mapping session (one handle of
 * each of those tables while it is open); their kernels do the cutting and the sweep, unchanged.
 * The definition.  Per slot, since its reset, lev[0 .. E) are the levels of the events emitted so far,
 *     level = (double)sum / (double)length of the event record.  The slot is in one of three states.
 *     CALIBRATING (after a reset): nothing has been mapped.  After a push, with E events in all and `ended` the END flag
 *         of this or an earlier push: if E < C and not ended the new levels are held back (held = E).  Otherwise
 *         head = lev[0 .. min(C, E)); with fewer than 2 levels in head, or not (sd > 0), the slot becomes UNDECIDABLE
 *         (mean = sd = NaN); otherwise mean = the sum of head in numpy's add.reduce order / n and
 *         sd = sqrt(sum((x - mean) * (x - mean)) / n) in the same order -- np.mean and np.std bit for bit -- the slot
 *         becomes MAPPING and the chunk handed to the mapping side is (lev[0 .. E) - mean) / sd, held levels first.
 *     MAPPING: the chunk is (new levels - mean) / sd; mean and sd stay until the reset.
 *     UNDECIDABLE: events are still cut and counted, nothing is mapped until the reset.
 *     One divide, one subtract and one divide per level, each correctly rounded: no tolerance anywhere.
 * A push: the event session's push of the sample chunks (its rules for len, END and ended slots), the bridge above, the
 *     mapping session's push of the chunks the bridge made, the summary.  out[t * m + k] is sk_map_push's record of slot
 *     slots[k] against target t: (dist, start, end, n, flags) of sk_dtw_subsequence(every normalised level the slot has
 *     been handed, target t) bit for bit, rows the number of those levels, pushes the pushes that handed at least one; a
 *     slot that has been handed nothing has dist NaN, start = end = -1, rows = pushes = 0.  info[k] is the slot's state
 *     after the push (events = E, mapped = levels handed so far, new_events = events this push cut).
 * The summary (rule != NULL): best[k] from the records of entry k, with d[t] = dist, NaN replaced by +inf: target = the
 *     first t of the smallest d[t], -1 when every dist is NaN; dist, start, end, rows are that record's (NaN, -1, -1 and
 *     record 0's rows without a target); second_target = the first t of the smallest d over the others (the best set to
 *     +inf: 0 when all are +inf), -1 with one target; second_dist = that record's dist as it stands (NaN with one
 *     target).  decision 1 (accept) when there is a target, rows >= min_rows, dist / rows <= max_dist_per_row and, with
 *     more than one target, (d[second_target] - dist) / rows >= min_margin; -1 (give up) when there is a target, it is
 *     not accepted and rows >= give_up_rows; 0 (wait) otherwise.
 * sk_live_fetch: the normalised chunks of the last push, compact: off [m + 1] always, values when off[m] <= cap
 *     (SK_ERR_OVERFLOW otherwise, off still complete); before the first push nothing is written.
 * sk_live_hits: sk_map_hits on the inner mapping session.  sk_live_reset: the slots start a new read (CALIBRATING).
 * Limits: SK_LIVE_MAX_SESSIONS per context, calib in 2 .. SK_LIVE_MAX_CALIB, nslots in 1 .. SK_MAP_MAX_SLOTS, the
 *     targets' limits of sk_map_open.  sk_shutdown closes open sessions.
 * Refusals (SK_ERR_INVALID unless said otherwise).  Those the arguments alone decide come before a context is looked
 *     for: at open sk_evs_open's for p and handle, calib outside its range, then sk_map_open's for the targets and
 *     nslots; at a push sk_evs_push_i16's (without off / rec / cap), NULL out / info, best without rule or rule without
 *     best, a rule with a NaN threshold or give_up_rows < 1.  Then the session: a handle that is not open, a slot outside
 *     [0, nslots), samples for an ended slot (host form), (calib - 1) + the event session's staging rows for `stride`
 *     above SK_MAP_MAX_CHUNK (SK_ERR_UNSUPPORTED).  A refused push changes nothing. */
#define SK_LIVE_MAX_SESSIONS 8
#define SK_LIVE_MAX_CALIB 8192      /* one numpy reduction buffer; 64 KB of hold buffer per slot at most */
enum { SK_LIVE_CALIBRATING = 0, SK_LIVE_MAPPING = 1, SK_LIVE_UNDECIDABLE = 2 };
typedef struct sk_live_info {       /* 40 bytes */
    double  mean, sd;               /* NaN until fixed, NaN when undecidable */
    int32_t events, mapped, held, state, ended, new_events;
} sk_live_info;
typedef struct sk_live_rule { int32_t min_rows, give_up_rows; double max_dist_per_row, min_margin; } sk_live_rule;
typedef struct sk_live_best {       /* 40 bytes */
    double  dist, second_dist;
    int32_t target, start, end, rows, second_target, decision;
} sk_live_best;
int sk_live_open(const sk_det_params *p, int32_t calib, const double *targets, const int64_t *target_off,
                 int32_t ntargets, int32_t nslots, int32_t *handle);
/* every pointer a host pointer; out [ntargets][m], info [m] and best [m] are complete when the call returns. */
int sk_live_push_i16(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride,
                     const int32_t *len, const int32_t *end /* may be NULL */, const sk_live_rule *rule /* may be NULL */,
                     sk_map_rec *out /* [ntargets][m] */, sk_live_info *info /* [m] */,
                     sk_live_best *best /* [m]; NULL iff rule NULL */);
/* device-resident form: slots, rows, len, end, out, info, best are device pointers, rule a host pointer.  The slot
 * numbers and the chunk lengths the bridge made are read back (the sweep is planned on the host); the slots are checked
 * against nslots and for doubles, len is clamped into [0, stride], samples for an ended slot are ignored. */
int sk_live_push_dev_i16(int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows, int64_t stride,
                         const int32_t *d_len, const int32_t *d_end /* may be NULL */, const sk_live_rule *rule /* may be NULL */,
                         sk_map_rec *d_out, sk_live_info *d_info, sk_live_best *d_best);
int sk_live_fetch(int32_t handle, int64_t *off /* [m + 1] */, double *values, int64_t cap);
int sk_live_hits(int32_t handle, const int32_t *slots, int32_t m, int32_t max_hits, double max_dist, sk_hit *out, int32_t *count);
int sk_live_reset(int32_t handle, const int32_t *slots, int32_t m);
int sk_live_close(int32_t handle);
/* The last push of a live session on the calling thread's context: bytes of slot state (both inner sessions' and
 * nslots * (calib * 8 + 40) of its own), the normalised levels the bridge handed to the mapping side, the kernels the
 * session launched itself (count, fill, summary) plus the sweep's launches.  Any pointer may be NULL. */
int sk_last_live_plan(int64_t *state_bytes, int64_t *bridged_levels, int64_t *launches);
/* Timing of the session's last push, when it was this context's last timed call: sk_last_kernel_ms gives prep = the
 * bridge (count, scan, fill) and main = the whole push from the event cutting to the summary, the read-back and the
 * host-side plan of the sweep included; this gives the bridge again and the summary kernel alone (0 without a rule). */
int sk_live_last_ms(int32_t handle, float *bridge_ms, float *summary_ms);

/* Gated live sessions: start at the transcript start an HMM gate finds (tests/livegate_ref.py states this in numpy).
 * A direct-RNA read begins with open pore, leader, adapter and poly(A): none of it belongs to a target, and all of it
 * would go into the calibration head.  A gated session is a live session plus one sk_hmm_model (checked and copied at
 * open as sk_hmms_open does; the session owns one HMM session handle beside its event and mapping handles), one gate
 * rule sk_live_gate, and per slot a gate record and a hold ring of the last G = hold events the slot was cut.
 * Reset: the slot is GATING, t0 = -1, the ring empty; the HMM slot is reset with the slot's calibration pair:
 *     sk_live_reset gives it none ({0.0, 1.0}), sk_live_reset_cal gives m {offset, unit} pairs as sk_hmms_reset takes them.
 * A push, per named slot:
 *     1. The chunk goes to the slot's HMM state only while the slot is GATING and has not ended; after the decision the
 *        HMM slot stands still, so its record stays the record at the decision.  The event session takes the chunk as in
 *        an ungated session, from sample 0.
 *     2. While GATING, api.polya_decide's rule on the slot's HMM record, expression for expression, `state` in place of
 *        TRANSCRIPT: accept when final_state == state and n_used - enter[state] >= min_body and
 *        v[state] - max(v[j], j != state) >= min_margin (the max over all six entries, -inf included; one float64
 *        subtract; a NaN margin fails).  On accept t0 = enter[state] and the slot is OPEN until its reset.  Otherwise,
 *        when give_up > 0 and n_used >= give_up, the slot is REJECTED.  Otherwise, when the push carries END, the slot is
 *        REJECTED with flag ENDED.  decided_n = n_used at any of the three.
 *     3. An event is released iff the slot is OPEN and event.start >= t0 (read coordinates): an event that straddles t0
 *        is dropped, whether it is emitted before or after the decision.  On the push that opens the gate the released
 *        events are those of the ring with start >= t0, oldest first, then those of this push with start >= t0; the
 *        events of that push do not pass through the ring.  While the slot stays GATING the events of the push are
 *        appended to the ring, which keeps the last G; TRUNCATED is set at the opening iff an event the ring had
 *        overwritten had start >= t0 (exact: the start of the most recently overwritten event is kept).  What is still
 *        held is released.  After the decision the ring is empty.
 *     4. The released events are the lev[0 .. E) of the definition above: sk_live_info's events, new_events, held and
 *        mapped count released events; END passes through unchanged, so a slot that ends while gating becomes
 *        UNDECIDABLE (fewer than 2 levels) and a give-up-rejected slot stays CALIBRATING with 0 events until it ends.
 *        Records, sk_live_fetch, sk_live_hits and the summary are those of the definition above over the released levels.
 * sk_live_push_i16 and sk_live_push_dev_i16 take gated handles as they are.  In the device form samples for an ended
 *     slot are ignored by both inner sessions.
 * sk_live_gate_fetch: the gate records and the HMM records of the entries of the last push (nothing before the first);
 *     either pointer may be NULL.  sk_live_gate_fetch_dev: the same to device pointers, a stream-ordered copy with
 *     nothing synchronised.
 * Limits: hold in 1 .. SK_LIVE_MAX_GATE_HOLD; a slot takes at most 0x7fffff00 samples (the HMM session's cap,
 *     SK_ERR_UNSUPPORTED in the host form whatever the gate's state; the device form ignores what is beyond and counts
 *     the slot in sk_last_hmms_plan's guard_hits while it is gating).
 * Refusals (SK_ERR_INVALID unless said otherwise).  By the arguments alone, before a context is looked for: at open
 *     sk_live_open's in its order, then a NULL model or gate, a model that breaks sk_hmms_open's rules (its message),
 *     state outside [0, nstates), min_body < 1, hold outside its range, a NaN min_margin; at sk_live_reset_cal
 *     sk_live_reset's, then a cal2 that is NULL or not finite; at sk_live_gate_fetch a handle outside the table.  Then
 *     the session: sk_live_gate_fetch or sk_live_reset_cal on an ungated handle; a push whose (calib - 1) + hold + the
 *     event session's staging rows for `stride` exceed SK_MAP_MAX_CHUNK (SK_ERR_UNSUPPORTED).  A refused call changes
 *     nothing.
 * sk_last_live_plan's state_bytes add the HMM session's bytes and nslots * (hold * 24 + 40) (ring and slot record); its
 *     launches add 3 (the chunk lengths, the HMM push, the gate). */
#define SK_LIVE_MAX_GATE_HOLD 4096
enum { SK_LIVE_GATE_GATING = 0, SK_LIVE_GATE_OPEN = 1, SK_LIVE_GATE_REJECTED = 2 };
enum { SK_LIVE_GATE_TRUNCATED = 1, SK_LIVE_GATE_ENDED = 2 };
typedef struct sk_live_gate {       /* 24 bytes */
    int32_t state, min_body, give_up, hold;
    double  min_margin;
} sk_live_gate;
typedef struct sk_live_gate_info {  /* 32 bytes */
    int32_t state, t0, decided_n, events_cut, released, ring, dropped, flags;
} sk_live_gate_info;
int sk_live_open_gated(const sk_det_params *p, int32_t calib, const double *targets, const int64_t *target_off,
                       int32_t ntargets, int32_t nslots, const sk_hmm_model *model, const sk_live_gate *gate,
                       int32_t *handle);
int sk_live_reset_cal(int32_t handle, const int32_t *slots, int32_t m, const double *cal2 /* [m][2] */);
int sk_live_gate_fetch(int32_t handle, sk_live_gate_info *gate /* [m] or NULL */, sk_hmms_rec *rec /* [m] or NULL */);
int sk_live_gate_fetch_dev(int32_t handle, sk_live_gate_info *d_gate, sk_hmms_rec *d_rec);
/* Timing of a gated session's last push, from HIP events of its own: the HMM side (the chunk lengths and k_hmms_push) and
 * the gate (k_live_gate and the scan of the released counts).  In a gated push sk_live_last_ms's bridge includes the
 * gate.  Either pointer may be NULL; SK_ERR_INVALID on an ungated handle. */
int sk_live_gate_last_ms(int32_t handle, float *hmm_ms, float *gate_ms);

/* Reference pile-up: per-point event statistics over aligned reads (tests/pileup_ref.py states this in numpy).
 * sk_dtw_pairs_paths, sk_dtw_band and the mapping calls say which target points every query point (event) of a pair
 * covers.  The pile-up turns that table round: for every point of every target, the events that cover it, in the reading
 * order of the table, and their statistics.
 * Inputs: span_off [npairs + 1] and spans [nrows][2] in the layout of those calls -- the rows of pair p are
 *     span_off[p] .. span_off[p + 1], row e covers the target points a_e .. b_e, a_e < 0 is "no path"; value [nrows] the
 *     query point of the row (an event's normalised level), dwell [nrows] its samples (NULL: ones); target [npairs] the
 *     target the pair was aligned to (NULL: zeros; negative: the pair is left out), shift [npairs] added to both ends of
 *     every span of the pair (NULL: zeros; a pair traced against target[start : start + span] has shift = start), use
 *     [npairs] (NULL: all ones; 0 leaves the pair out); tlen [ntargets] the targets' lengths.  toff = their running sum:
 *     point j of target t has the flat index toff[t] + j, Mtot = toff[ntargets].
 * Entries: row e of pair p is USED when target[p] >= 0, use[p] != 0 and a_e >= 0; a used row is one entry of every point
 *     a_e + shift[p] .. b_e + shift[p] of target[p].  A point's list is ordered by ascending row index.
 * out [Mtot], one sk_pile_rec per flat point; with v = value and d = dwell over the point's list, in order, numpy's
 *     expressions and its order of summation (np.add.reduce: buffers of 8 192 terms, the pairwise tree inside one), bit
 *     for bit:
 *         level = np.mean(v)   level_sd = np.std(v)   vmin = np.min(v)   vmax = np.max(v)
 *         dwell_mean = np.sum(d, dtype=int64) / n     dwell_sd = np.std(d.astype(float64))
 *         n = entries   depth = distinct pairs among them   shared = entries whose row covers more than one point
 *     A point without entries has six NaN doubles (0x7FF8000000000000) and three zeros.  A NaN among v gives NaN in the
 *     four statistics of v: the first NaN of the list, quieted.  A NaN that the arithmetic itself makes (inf - inf) has
 *     the bits 0xFFF8000000000000, which is what numpy gives on an x86-64 host; a list that holds both a NaN and such
 *     a sum gets the list's NaN.  When a list holds both zeros the sign of a zero vmin / vmax is not defined.  No field
 *     is formed with floating-point atomics: two calls give the same bytes.
 * ent_off [Mtot + 1], ent_row [ent_cap] (both NULL, or both set): the inverted index itself -- the rows of flat point m
 *     are ent_row[ent_off[m] .. ent_off[m + 1]), ascending.  ent_off[Mtot] = the sum of b_e - a_e + 1 over the used rows.
 * Refusals (SK_ERR_INVALID), checked before anything is written to out / ent_off / ent_row.  By the arguments alone:
 *     npairs, nrows or ntargets negative, a NULL out / tlen / span_off, NULL spans / value with nrows > 0, one of ent_off
 *     / ent_row without the other, a negative ent_cap, a negative tlen (the target is named).  Then on the device, the
 *     lowest offending pair index named in sk_last_error() whatever the launch order: span_off[0] != 0, span_off not
 *     non-decreasing (the pair whose range ends before it begins), span_off[npairs] != nrows -- these three first, since
 *     they decide which pair a row belongs to; then target[p] >= ntargets (whether or not the pair is used), a used row
 *     with b_e < a_e, a used row whose shifted span leaves [0, tlen[t]).  Then ent_cap below the number of entries.
 *     npairs == 0 or nrows == 0 is SK_OK with every record the empty one; tlen == 0 is legal.
 * Limits: nrows <= 2^31 - 1, Mtot <= 2^40, entries per point <= 2^31 - 1, entries in all <= 2^40 (SK_ERR_UNSUPPORTED
 *     with the limit named); device memory per entry 4 bytes, 8 when a list takes the merge tier; 16 bytes per point and
 *     4 per row beside them (SK_ERR_NOMEM when it does not fit).
 * sk_pileup: every pointer a host pointer.  sk_pileup_dev: device pointers but tlen, which stays on the host (the
 *     convention of sk_dtw_pairs_paths_dev); it synchronises once, to read the checks' verdict and the entry count.
 * sk_last_pileup_plan: the last such call on this context -- entries, the longest list, the lists that took the merge
 *     tier, bytes of device scratch; any pointer may be NULL. */
typedef struct sk_pile_rec {        /* 64 bytes */
    double  level, level_sd, vmin, vmax, dwell_mean, dwell_sd;
    int32_t depth, n, shared, pad;
} sk_pile_rec;
int sk_pileup(const int64_t *span_off, const int32_t *spans, const double *value, const int32_t *dwell,
              const int32_t *target, const int32_t *shift, const uint8_t *use, int32_t npairs, int64_t nrows,
              const int64_t *tlen, int32_t ntargets, sk_pile_rec *out, int64_t *ent_off, int32_t *ent_row, int64_t ent_cap);
int sk_pileup_dev(const int64_t *d_span_off, const int32_t *d_spans, const double *d_value, const int32_t *d_dwell,
                  const int32_t *d_target, const int32_t *d_shift, const uint8_t *d_use, int32_t npairs, int64_t nrows,
                  const int64_t *tlen, int32_t ntargets, sk_pile_rec *d_out, int64_t *d_ent_off, int32_t *d_ent_row,
                  int64_t ent_cap);
int sk_last_pileup_plan(int64_t *entries, int64_t *longest_list, int64_t *lists_in_long_tier, int64_t *scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SQUIGGLEKIT_HIP_H */
