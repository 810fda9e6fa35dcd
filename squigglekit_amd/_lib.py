"""ctypes binding of libsquigglekit_hip.so (the C ABI in include/squigglekit_hip.h).

There is no CPU fallback: if the shared library is missing, or no gfx950 device is
visible, every compute call raises.  Nothing here imports torch or the oracle.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("SK_LIB_PATH") or os.path.join(_HERE, "libsquigglekit_hip.so")   # (override: A/B builds)
CSRC = os.path.join(_HERE, "csrc")


class SquiggleKitError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("squigglekit_hip error %d: %s" % (code, msg))
        self.code = code


# sk_status (include/squigglekit_hip.h)
SK_OK, SK_ERR_INVALID, SK_ERR_NO_DEVICE, SK_ERR_HIP, SK_ERR_NOMEM, SK_ERR_UNSUPPORTED, SK_ERR_OVERFLOW = 0, -1, -2, -3, -4, -5, -6
SK_SCALE = {"medmad": 0, "zscale": 1}
SK_PULL_RAW, SK_PULL_PA = 0, 1
SK_FLAG_EMPTY, SK_FLAG_DEGENERATE, SK_FLAG_RECENTRE = 1, 2, 4
SK_PAIRS_SUBSEQUENCE, SK_PAIRS_GLOBAL = 0, 1
SK_BAND_PINNED, SK_BAND_FREE = 0, 1
SK_FLAG_BAND_LOST = 16                  # sk_dtw_band: the band lost the end cell (dist = +inf)
SK_FLAG_CALIBRATING = 8                 # sk_stream_rec.flags: the slot still collects its calibration samples
SK_STREAM_MAX_CALIB, SK_STREAM_MAX_SLOTS, SK_STREAM_MAX_POINTS = 65536, 65536, 1024


class SegParams(C.Structure):
    """sk_seg_params; defaults are the argparse defaults of segmenter.py:65-96."""
    _fields_ = [("error", C.c_int32), ("corrector", C.c_int32), ("window", C.c_int32),
                ("seg_dist", C.c_int32), ("std_scale", C.c_double), ("stall_len", C.c_double),
                ("lim_low", C.c_int32), ("lim_hi", C.c_int32)]

    def __init__(self, error=5, corrector=50, window=150, seg_dist=50, std_scale=0.75,
                 stall_len=0.25, lim_low=0, lim_hi=900):
        super().__init__(error, corrector, window, seg_dist, std_scale, stall_len, lim_low, lim_hi)

    @classmethod
    def from_args(cls, args):
        """Build from an argparse Namespace shaped like segmenter.py's."""
        return cls(args.error, args.corrector, args.window, args.seg_dist, args.std_scale,
                   args.stall_len, getattr(args, "lim_low", 0), getattr(args, "lim_hi", 900))


class SweepSet(C.Structure):
    """sk_seg_sweep_set: one parameter set of a sweep -- the segmenter's flags plus the -j / -b test thresholds."""
    _fields_ = [("seg", SegParams), ("stall_start", C.c_int32), ("gap_dist", C.c_int32)]

    def __init__(self, seg=None, stall_start=300, gap_dist=3000):
        super().__init__(seg if seg is not None else SegParams(), stall_start, gap_dist)


class SweepRec(C.Structure):
    """sk_seg_sweep_rec: one (set, read) of a sweep."""
    _fields_ = [("nsegs", C.c_int32), ("s0_start", C.c_int32), ("s0_end", C.c_int32),
                ("s1_start", C.c_int32), ("s1_end", C.c_int32), ("reserved", C.c_int32)]


class SweepSum(C.Structure):
    """sk_seg_sweep_sum: one set's counts over the reads."""
    _fields_ = [("reads", C.c_int64), ("with_segs", C.c_int64), ("segs", C.c_int64), ("stall_ok", C.c_int64),
                ("gap_ok", C.c_int64), ("stall_gap_ok", C.c_int64), ("seg0_end_sum", C.c_int64), ("reserved", C.c_int64)]


SWEEP_REC_DTYPE = np.dtype([(n, "<i4") for n, _ in SweepRec._fields_])
SWEEP_SUM_DTYPE = np.dtype([(n, "<i8") for n, _ in SweepSum._fields_])


class DrnaParams(C.Structure):
    """sk_drna_params; defaults are the constants hard-coded at dRNA_segmenter.py:80-104."""
    _fields_ = [("error", C.c_int32), ("no_err_thresh", C.c_int32), ("w", C.c_int32),
                ("window", C.c_int32), ("seg_dist", C.c_int32), ("t_start", C.c_int32),
                ("t_end", C.c_int32), ("std_scale", C.c_double), ("lim_low", C.c_int32),
                ("lim_hi", C.c_int32)]

    def __init__(self, error=5, no_err_thresh=2500, w=1200, window=100, seg_dist=1200, t_start=1000,
                 t_end=5000, std_scale=0.8, lim_low=0, lim_hi=1200):
        super().__init__(error, no_err_thresh, w, window, seg_dist, t_start, t_end, std_scale,
                         lim_low, lim_hi)


class RollParams(C.Structure):
    """sk_roll_params: the constants of dRNA_segmenter.py:288-295,322 and the rolling window `w` the
    script reads before assigning (its commented-out default, :81, is 2000)."""
    _fields_ = [("w", C.c_int32), ("seg_dist", C.c_int32), ("hi_thresh", C.c_int32), ("lo_thresh", C.c_int32),
                ("shift", C.c_int32), ("std_scale", C.c_double), ("lim_low", C.c_int32), ("lim_hi", C.c_int32)]

    def __init__(self, w=2000, seg_dist=1500, hi_thresh=200000, lo_thresh=2000, shift=1000, std_scale=0.5,
                 lim_low=0, lim_hi=1200):
        super().__init__(w, seg_dist, hi_thresh, lo_thresh, shift, std_scale, lim_low, lim_hi)


class SynthOpts(C.Structure):
    """sk_synth_opts (bench tooling): slice / variant of the device generator's batch."""
    _fields_ = [("row0", C.c_int64), ("hit_permille", C.c_int32), ("stretch_permille", C.c_int32),
                ("stretch", C.c_int32), ("tmpl", C.c_void_p), ("ntmpl", C.c_int32), ("tmpl_noise", C.c_double)]

    def __init__(self, row0=0, hit_permille=500, stretch_permille=0, stretch=1, tmpl=None, tmpl_noise=0.0):
        self._keep = None if tmpl is None else np.ascontiguousarray(tmpl, dtype=np.int16)
        super().__init__(row0, hit_permille, stretch_permille, stretch,
                         None if tmpl is None else self._keep.ctypes.data, 0 if tmpl is None else self._keep.size,
                         tmpl_noise)


class Hit(C.Structure):
    _fields_ = [("dist", C.c_double), ("start", C.c_int32), ("end", C.c_int32),
                ("n", C.c_int32), ("flags", C.c_int32)]


HIT_DTYPE = np.dtype([("dist", "<f8"), ("start", "<i4"), ("end", "<i4"),
                      ("n", "<i4"), ("flags", "<i4")])



class PanelRec(C.Structure):
    """sk_panel_rec: one read of a motif panel -- the two best motifs by score and the best one's record."""
    _fields_ = [("best", C.c_int32), ("second", C.c_int32), ("score_best", C.c_double), ("score_second", C.c_double),
                ("hit", Hit)]


PANEL_DTYPE = np.dtype([("best", "<i4"), ("second", "<i4"), ("score_best", "<f8"), ("score_second", "<f8"),
                        ("hit", HIT_DTYPE)])


class BgRec(C.Structure):
    """sk_bg_rec: the statistics of one read's whole last DTW row against one motif (MotifSeq.py:507-513)."""
    _fields_ = [("mean", C.c_double), ("std", C.c_double), ("median", C.c_double), ("mad", C.c_double),
                ("below", C.c_int32), ("n", C.c_int32), ("reserved", C.c_int32 * 2)]


# the six fields of the 48-byte record (its two reserved words are not exposed)
BG_DTYPE = np.dtype({"names": ["mean", "std", "median", "mad", "below", "n"],
                     "formats": ["<f8", "<f8", "<f8", "<f8", "<i4", "<i4"],
                     "offsets": [0, 8, 16, 24, 32, 36], "itemsize": 48})

class Event(C.Structure):
    """sk_event: what the signal did in the samples of one motif point of one hit."""
    _fields_ = [("sum", C.c_double), ("std", C.c_double), ("cost", C.c_double), ("start", C.c_int32), ("dwell", C.c_int32)]


EVENT_DTYPE = np.dtype([("sum", "<f8"), ("std", "<f8"), ("cost", "<f8"), ("start", "<i4"), ("dwell", "<i4")])


class PoolRec(C.Structure):
    """sk_pool_rec: one motif point of the model the pooled hits show."""
    _fields_ = [("level", C.c_double), ("level_sd", C.c_double), ("sd_mean", C.c_double), ("dwell_mean", C.c_double),
                ("dwell_sd", C.c_double), ("cost_mean", C.c_double), ("hits", C.c_int32), ("pad", C.c_int32)]


# the seven fields of the 56-byte record (its pad word is not exposed)
POOL_DTYPE = np.dtype({"names": ["level", "level_sd", "sd_mean", "dwell_mean", "dwell_sd", "cost_mean", "hits"],
                       "formats": ["<f8"] * 6 + ["<i4"], "offsets": [0, 8, 16, 24, 32, 40, 48], "itemsize": 56})

class SegLevel(C.Structure):
    """sk_seg_level: what the signal did in one segment (or in the whole filtered read), and where it lies in the raw read."""
    _fields_ = [("mean", C.c_double), ("std", C.c_double), ("median", C.c_double), ("mad", C.c_double),
                ("min", C.c_double), ("max", C.c_double), ("raw_start", C.c_int32), ("raw_end", C.c_int32),
                ("n", C.c_int32), ("pad", C.c_int32)]


LEVEL_DTYPE = np.dtype([("mean", "<f8"), ("std", "<f8"), ("median", "<f8"), ("mad", "<f8"), ("min", "<f8"), ("max", "<f8"),
                        ("raw_start", "<i4"), ("raw_end", "<i4"), ("n", "<i4"), ("pad", "<i4")])

class DetParams(C.Structure):
    """sk_det_params: windows, thresholds and peak height of event detection (the header's "event detection" section
    states the definition); the defaults are its dna preset."""
    _fields_ = [("w_short", C.c_int32), ("w_long", C.c_int32), ("th_short", C.c_double), ("th_long", C.c_double),
                ("peak_height", C.c_double)]

    def __init__(self, w_short=3, w_long=6, th_short=1.4, th_long=9.0, peak_height=0.2):
        super().__init__(w_short, w_long, th_short, th_long, peak_height)


class DetEvent(C.Structure):
    """sk_det_event: one event [start, start + length) of a read in raw coordinates, with the exact sum and sum of squares
    of its samples."""
    _fields_ = [("start", C.c_int32), ("length", C.c_int32), ("sum", C.c_int64), ("sumsq", C.c_int64)]


DET_EVENT_DTYPE = np.dtype([("start", "<i4"), ("length", "<i4"), ("sum", "<i8"), ("sumsq", "<i8")])


SK_HMM_STATES = 6


class HmmModel(C.Structure):
    """sk_hmm_model: a signal HMM of up to six states with two emission components each, as plain doubles (the header's
    "signal HMM" section states the definition; api.hmm_model builds one from probabilities)."""
    _fields_ = [("nstates", C.c_int32), ("reserved", C.c_int32), ("linit", C.c_double * SK_HMM_STATES),
                ("ltrans", (C.c_double * SK_HMM_STATES) * SK_HMM_STATES), ("c", (C.c_double * 2) * SK_HMM_STATES),
                ("mu", (C.c_double * 2) * SK_HMM_STATES), ("h", (C.c_double * 2) * SK_HMM_STATES)]

    @classmethod
    def from_arrays(cls, nstates, linit, ltrans, c, mu, h):
        """The model of the given numbers, unchecked (the library checks): linit [S], ltrans [S, S], c / mu / h [S, 2] for
        S = len(linit); nstates may differ from S only to build a model the library must refuse."""
        m = cls()
        m.nstates = int(nstates)
        linit, ltrans = np.asarray(linit, dtype=np.float64), np.asarray(ltrans, dtype=np.float64)
        S = linit.size
        if S > SK_HMM_STATES or ltrans.shape != (S, S):
            raise ValueError("need linit [S] and ltrans [S, S] with S <= %d" % SK_HMM_STATES)
        m.linit[:] = [float("-inf")] * SK_HMM_STATES
        for i in range(SK_HMM_STATES):
            m.ltrans[i][:] = [float("-inf")] * SK_HMM_STATES
            m.c[i][:] = [float("-inf")] * 2
        for name, a in (("c", c), ("mu", mu), ("h", h)):
            a = np.asarray(a, dtype=np.float64)
            if a.shape != (S, 2):
                raise ValueError("%s must be [S, 2]" % name)
            for j in range(S):
                getattr(m, name)[j][:] = [float(a[j, 0]), float(a[j, 1])]
        for i in range(S):
            m.linit[i] = float(linit[i])
            for j in range(S):
                m.ltrans[i][j] = float(ltrans[i, j])
        return m

    def arrays(self):
        """{"nstates", "linit" [6], "ltrans" [6, 6], "c" / "mu" / "h" [6, 2]} as numpy arrays"""
        return {"nstates": int(self.nstates), "linit": np.array(self.linit[:], dtype=np.float64),
                "ltrans": np.array([row[:] for row in self.ltrans], dtype=np.float64),
                "c": np.array([row[:] for row in self.c], dtype=np.float64),
                "mu": np.array([row[:] for row in self.mu], dtype=np.float64),
                "h": np.array([row[:] for row in self.h], dtype=np.float64)}


HMM_DTYPE = np.dtype([("score", "<f8"), ("final_state", "<i4"), ("n_used", "<i4"), ("enter", "<i4", (SK_HMM_STATES,))])
# sk_hmm_seg / sk_hmm_segf: a maximal run of one state on the best path (int16 feed: exact integers of the raw samples)
HMM_SEG_DTYPE = np.dtype([("state", "<i4"), ("start", "<i4"), ("length", "<i4"), ("n1", "<i4"), ("sum", "<i8", (2,)),
                          ("sumsq", "<i8", (2,))])
HMM_SEGF_DTYPE = np.dtype([("state", "<i4"), ("start", "<i4"), ("length", "<i4"), ("n1", "<i4"), ("sum", "<f8", (2,)),
                           ("sumsq", "<f8", (2,))])
# sk_hmm_post / sk_hmm_counts: a read's posterior record (112 bytes) and its soft counts (624 bytes)
SK_HMM_POST_IMPOSSIBLE = 1
HMM_POST_DTYPE = np.dtype([("loglik", "<f8"), ("n_used", "<i4"), ("flags", "<i4"), ("final_post", "<f8", (SK_HMM_STATES,)),
                           ("occ", "<f8", (SK_HMM_STATES,))])
HMM_COUNTS_DTYPE = np.dtype([("n", "<f8", (SK_HMM_STATES, 2)), ("sx", "<f8", (SK_HMM_STATES, 2)),
                             ("sxx", "<f8", (SK_HMM_STATES, 2)), ("xi", "<f8", (SK_HMM_STATES, SK_HMM_STATES)),
                             ("init", "<f8", (SK_HMM_STATES,))])

class StreamParams(C.Structure):
    """sk_stream_params: what a MotifSeq session is opened with."""
    _fields_ = [("scale_mode", C.c_int32), ("scale_low", C.c_int32), ("scale_hi", C.c_int32), ("calib", C.c_int32),
                ("nslots", C.c_int32), ("reserved", C.c_int32 * 3)]


class StreamRec(C.Structure):
    """sk_stream_rec: one slot's record against one motif after a push."""
    _fields_ = [("dist", C.c_double), ("tail", C.c_double), ("start", C.c_int32), ("end", C.c_int32), ("n", C.c_int32),
                ("seen", C.c_int32), ("flags", C.c_int32), ("chunks", C.c_int32)]


STREAM_DTYPE = np.dtype([("dist", "<f8"), ("tail", "<f8"), ("start", "<i4"), ("end", "<i4"), ("n", "<i4"), ("seen", "<i4"),
                         ("flags", "<i4"), ("chunks", "<i4")])

# sk_map_rec: one slot's record against one target after a push of a mapping session (sk_hit's fields, then the counters)
MAPREC_DTYPE = np.dtype([("dist", "<f8"), ("start", "<i4"), ("end", "<i4"), ("n", "<i4"), ("flags", "<i4"), ("rows", "<i4"),
                         ("pushes", "<i4")])
SK_MAP_MAX_SESSIONS, SK_MAP_MAX_SLOTS, SK_MAP_MAX_TARGETS, SK_MAP_MAX_CHUNK = 8, 65536, 65536, 65536
SK_MAP_MAX_STATE_BYTES = 1 << 35
SK_EVS_MAX_SESSIONS, SK_EVS_MAX_SLOTS = 8, 1048576
SK_HMMS_MAX_SESSIONS, SK_HMMS_MAX_SLOTS, SK_HMMS_MAX_SAMPLES = 8, 1048576, 0x7fffff00
SK_LIVE_MAX_SESSIONS, SK_LIVE_MAX_CALIB = 8, 8192
SK_LIVE_CALIBRATING, SK_LIVE_MAPPING, SK_LIVE_UNDECIDABLE = 0, 1, 2
# sk_live_info: a live session's slot after a push; sk_live_best: the decision summary of one entry (40 bytes each)
LIVEINFO_DTYPE = np.dtype([("mean", "<f8"), ("sd", "<f8"), ("events", "<i4"), ("mapped", "<i4"), ("held", "<i4"),
                           ("state", "<i4"), ("ended", "<i4"), ("new_events", "<i4")])
LIVEBEST_DTYPE = np.dtype([("dist", "<f8"), ("second_dist", "<f8"), ("target", "<i4"), ("start", "<i4"), ("end", "<i4"),
                           ("rows", "<i4"), ("second_target", "<i4"), ("decision", "<i4")])


class LiveRule(C.Structure):
    """sk_live_rule: api.map_decide's thresholds, for the decision summary of a live session's push."""
    _fields_ = [("min_rows", C.c_int32), ("give_up_rows", C.c_int32), ("max_dist_per_row", C.c_double),
                ("min_margin", C.c_double)]


# gated live sessions: sk_live_gate (the rule, 24 bytes) and sk_live_gate_info (a slot's gate record, 32 bytes)
SK_LIVE_MAX_GATE_HOLD = 4096
SK_LIVE_GATE_GATING, SK_LIVE_GATE_OPEN, SK_LIVE_GATE_REJECTED = 0, 1, 2
SK_LIVE_GATE_TRUNCATED, SK_LIVE_GATE_ENDED = 1, 2
GATE_DTYPE = np.dtype([("state", "<i4"), ("t0", "<i4"), ("decided_n", "<i4"), ("events_cut", "<i4"), ("released", "<i4"),
                       ("ring", "<i4"), ("dropped", "<i4"), ("flags", "<i4")])


class PileRec(C.Structure):
    """sk_pile_rec: one flat reference point of a pile-up (64 bytes)."""
    _fields_ = [("level", C.c_double), ("level_sd", C.c_double), ("vmin", C.c_double), ("vmax", C.c_double),
                ("dwell_mean", C.c_double), ("dwell_sd", C.c_double), ("depth", C.c_int32), ("n", C.c_int32),
                ("shared", C.c_int32), ("pad", C.c_int32)]


PILE_DTYPE = np.dtype([("level", "<f8"), ("level_sd", "<f8"), ("vmin", "<f8"), ("vmax", "<f8"), ("dwell_mean", "<f8"),
                       ("dwell_sd", "<f8"), ("depth", "<i4"), ("n", "<i4"), ("shared", "<i4"), ("pad", "<i4")])


class LiveGate(C.Structure):
    """sk_live_gate: api.polya_decide's thresholds with the state whose entry is the start, and the hold ring's length."""
    _fields_ = [("state", C.c_int32), ("min_body", C.c_int32), ("give_up", C.c_int32), ("hold", C.c_int32),
                ("min_margin", C.c_double)]

# sk_hmms_rec: a slot's record after a push of an HMM session -- sk_hmm_rec's 40 bytes, then the six scores and the counters
HMMS_DTYPE = np.dtype([("score", "<f8"), ("final_state", "<i4"), ("n_used", "<i4"), ("enter", "<i4", (SK_HMM_STATES,)),
                       ("v", "<f8", (SK_HMM_STATES,)), ("pushes", "<i4"), ("flags", "<i4")])
# sk_hmms_filt: a slot's filter in a session opened with SK_HMMS_FILTER -- loglik and P(state at the newest sample)
SK_HMMS_FILTER = 1
HMMS_FILT_DTYPE = np.dtype([("loglik", "<f8"), ("n_used", "<i4"), ("flags", "<i4"), ("post", "<f8", (SK_HMM_STATES,))])

# every symbol include/squigglekit_hip.h declares: name -> (restype, argtypes)
_vp, _i16p, _i32p, _i64p, _dp = (C.c_void_p, C.POINTER(C.c_int16), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int64), C.POINTER(C.c_double))
# the hit family (hit lists, background, paths, events): its int16 and its ragged forms share an argument list up to
# out, count; background, paths and events add one output
_HITS_TAIL = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, _vp, _vp]
_HITS_I16 = [_vp, C.c_int64, _vp, C.c_int32] + _HITS_TAIL
_HITS_RAGGED = [_vp, _vp, C.c_int32] + _HITS_TAIL
ABI = {
    "sk_version": (C.c_char_p, []),
    "sk_last_error": (C.c_char_p, []),
    "sk_device_count": (C.c_int, []),
    "sk_init": (C.c_int, [C.c_int]),
    "sk_init_slot": (C.c_int, [C.c_int, C.c_int]),
    "sk_shutdown": (C.c_int, []),
    "sk_sync": (C.c_int, []),
    "sk_device_name": (C.c_int, [C.c_char_p, C.c_int]),
    "sk_device_pci_bus_id": (C.c_int, [C.c_char_p, C.c_int]),
    "sk_dev_alloc": (_vp, [C.c_size_t]),
    "sk_dev_free": (C.c_int, [_vp]),
    "sk_dev_upload": (C.c_int, [_vp, _vp, C.c_size_t]),
    "sk_dev_download": (C.c_int, [_vp, _vp, C.c_size_t]),
    "sk_host_alloc": (_vp, [C.c_size_t]),
    "sk_host_free": (C.c_int, [_vp]),
    "sk_segment_batch_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.POINTER(SegParams),
                                       _vp, _vp, C.c_int32]),
    "sk_segment_batch_f64": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(SegParams), _vp, _vp, C.c_int32]),
    "sk_segment_batch_i16_pa": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.POINTER(SegParams), _vp, _vp, C.c_int32]),
    "sk_pa_calib": (C.c_int, [_vp, C.c_int32, _vp]),
    "sk_segment_dev_i16_pa": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.POINTER(SegParams), _vp, _vp, C.c_int32]),
    "sk_last_pa_retries": (C.c_int, []),
    "sk_segment_batch_f64_len": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.POINTER(SegParams), _vp, _vp, C.c_int32]),
    "sk_segment_batch_centi_len": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.POINTER(SegParams), _vp, _vp, C.c_int32]),
    "sk_segment_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.POINTER(SegParams),
                                     _vp, _vp, C.c_int32]),
    "sk_segment_dev_f64": (C.c_int, [_vp, _vp, C.c_int32, C.c_int64, C.c_int64, C.POINTER(SegParams), _vp, _vp, C.c_int32]),
    "sk_segment_levels_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.POINTER(SegParams), _vp, _vp, C.c_int32, _vp, _vp]),
    "sk_segment_levels_f64_len": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.POINTER(SegParams), _vp, _vp, C.c_int32, _vp, _vp]),
    "sk_segment_levels_centi_len": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.POINTER(SegParams), _vp, _vp, C.c_int32, _vp, _vp]),
    "sk_segment_levels_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.POINTER(SegParams), _vp, _vp, C.c_int32, _vp, _vp]),
    "sk_drna_segment_batch_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp, C.c_int32]),
    "sk_drna_roll_batch_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp]),
    "sk_drna_segment_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp, C.c_int32]),
    "sk_drna_roll_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp]),
    "sk_motifseq_batch_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, _vp]),
    "sk_motifseq_multi_batch_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_int32, _vp]),
    "sk_motifseq_batch_f64": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, _vp]),
    "sk_motifseq_multi_batch_f64": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp]),
    "sk_motifseq_multi_batch_centi": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp]),
    "sk_motifseq_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, _vp]),
    "sk_motifseq_multi_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, _vp]),
    "sk_motifseq_hits_i16": (C.c_int, _HITS_I16),
    "sk_motifseq_hits_f64": (C.c_int, _HITS_RAGGED),
    "sk_motifseq_hits_centi": (C.c_int, _HITS_RAGGED),
    "sk_motifseq_hits_dev_i16": (C.c_int, _HITS_I16),
    "sk_motifseq_background_i16": (C.c_int, _HITS_I16 + [_vp]),
    "sk_motifseq_background_f64": (C.c_int, _HITS_RAGGED + [_vp]),
    "sk_motifseq_background_centi": (C.c_int, _HITS_RAGGED + [_vp]),
    "sk_motifseq_background_dev_i16": (C.c_int, _HITS_I16 + [_vp]),
    "sk_motifseq_paths_i16": (C.c_int, _HITS_I16 + [_vp]),
    "sk_motifseq_paths_f64": (C.c_int, _HITS_RAGGED + [_vp]),
    "sk_motifseq_paths_centi": (C.c_int, _HITS_RAGGED + [_vp]),
    "sk_motifseq_paths_dev_i16": (C.c_int, _HITS_I16 + [_vp]),
    "sk_motifseq_events_i16": (C.c_int, _HITS_I16 + [_vp]),
    "sk_motifseq_events_f64": (C.c_int, _HITS_RAGGED + [_vp]),
    "sk_motifseq_events_centi": (C.c_int, _HITS_RAGGED + [_vp]),
    "sk_motifseq_events_dev_i16": (C.c_int, _HITS_I16 + [_vp]),
    "sk_events_pool": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _vp]),
    "sk_events_pool_dev": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _vp]),
    "sk_last_path_mismatches": (C.c_int, []),
    "sk_motifseq_panel_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32,
                                        _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "sk_motifseq_panel_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32,
                                            _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "sk_motifseq_panel_f64": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32,
                                        _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "sk_region_rows_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int64, _vp, _vp, _vp]),
    "sk_dtw_subsequence_path": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _dp, _i32p, _i32p, _vp]),
    "sk_motifseq_dev_f64": (C.c_int, [_vp, _vp, C.c_int32, C.c_int64, C.c_int64, _vp, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, _vp]),
    "sk_dtw_subsequence_batch": (C.c_int, [_vp, C.c_int32, _vp, _vp, C.c_int32, _vp]),
    "sk_dtw_subsequence": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _dp, _i32p, _i32p, _vp]),
    # DTW over a pair list: values, off, nseq, pairs [npairs] of {query, target}, npairs, mode, out [npairs] -- the
    # device-resident form takes the same list (values / out device, off / pairs host)
    "sk_dtw_pairs": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int64, C.c_int32, _vp]),
    "sk_dtw_pairs_dev": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int64, C.c_int32, _vp]),
    # ... and its warping paths: the same list, then records, have_records, spans [sum N][2]
    "sk_dtw_pairs_paths": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int64, C.c_int32, _vp, C.c_int32, _vp]),
    "sk_dtw_pairs_paths_dev": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int64, C.c_int32, _vp, C.c_int32, _vp]),
    "sk_last_pair_paths_tiers": (C.c_int, [_vp, _vp, _vp]),
    # adaptive-band DTW over the same list: band, end_mode, records, spans [sum N][2] or NULL (records only)
    "sk_dtw_band": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, _vp]),
    "sk_dtw_band_dev": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, _vp]),
    "sk_last_band_plan": (C.c_int, [_vp, _vp, _vp]),
    "sk_dtw_subsequence_cref": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _dp, _i32p, _i32p]),
    "sk_normalise_i16": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _i32p]),
    "sk_normalise_f64": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _i32p]),
    "sk_tsv_count_lines": (C.c_int64, [_vp, C.c_size_t]),
    "sk_tsv_count_tokens": (C.c_int, [_vp, C.c_size_t, C.c_int32, C.c_int64, _vp, C.c_int32]),
    "sk_tsv_parse": (C.c_int, [_vp, C.c_size_t, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                               C.c_int32]),
    "sk_tsv_parse_centi": (C.c_int, [_vp, C.c_size_t, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     C.c_int32]),
    "sk_tsv_parse_i16": (C.c_int, [_vp, C.c_size_t, C.c_int32, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, C.c_int32]),
    "sk_fmt_rows": (_vp, [C.c_int64, C.c_int32, _vp, _vp, C.c_int32, _i64p]),
    "sk_fmt_free": (None, [_vp]),
    "sk_ndtr": (None, [_vp, _vp, C.c_int64]),
    "sk_blow5_index": (C.c_int64, [_vp, C.c_int64, C.c_int64, _vp, _vp, C.c_int64]),
    "sk_blow5_index_some": (C.c_int64, [_vp, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp]),
    "sk_blow5_rows_i16": (C.c_int, [_vp, C.c_int64, _vp, _vp, C.c_int64, C.c_int32, C.c_int64, _vp, _vp, _vp, C.c_int32, _vp, _vp,
                                    C.c_int32]),
    "sk_comm_unique_id": (C.c_int, [_vp]),
    "sk_comm_init_rank": (C.c_int, [_vp, C.c_int, C.c_int]),
    "sk_comm_init_all": (C.c_int, [_i32p, C.c_int]),
    "sk_comm_info": (C.c_int, [_i32p, _i32p]),
    "sk_comm_allgather_dev": (C.c_int, [_vp, _vp, C.c_size_t]),
    "sk_comm_allgather_host": (C.c_int, [_vp, _vp, C.c_size_t]),
    "sk_comm_destroy": (C.c_int, []),
    "sk_tunables": (C.c_int, [C.c_char_p, C.c_int]),
    "sk_last_kernel_ms": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sk_last_dtw_retries": (C.c_int, []),
    "sk_last_dtw_tier2": (C.c_int, []),
    "sk_last_dtw_guard": (C.c_int, [_i32p]),
    "sk_last_dtw_window_steps": (C.c_int, [_vp]),
    "sk_last_dtw_premise_violations": (C.c_int, []),
    "sk_last_dtw_audit_mismatches": (C.c_int, []),
    "sk_last_f64_retries": (C.c_int, []),
    "sk_last_dtw_clock": (C.c_int, [_dp]),
    "sk_last_dtw_profile": (C.c_int, [C.POINTER(C.c_float), _i32p, C.POINTER(C.c_float), _i32p, _i32p]),
    "sk_synth_squiggles_dev": (C.c_int, [_vp, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, _vp, C.c_int32]),
    "sk_synth_variant_dev": (C.c_int, [_vp, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, _vp, C.c_int32, _vp]),
    "sk_synth_pa_dev": (C.c_int, [_vp, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, _vp, _vp]),
    "sk_pull_text": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, C.c_int64, _i64p, _vp]),
    "sk_segment_sweep_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp]),
    "sk_segment_sweep_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp]),
    "sk_segment_sweep_f64": (C.c_int, [_vp, _vp, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp]),
    "sk_pull_text_dev": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, C.c_int64, _i64p, _vp]),
    # event detection (the definition: "event detection" in include/squigglekit_hip.h and DESIGN.md; tests/detect_ref.py
    # states it in numpy): sig, stride, len, nreads, params, off [nreads + 1], rec, cap
    "sk_detect_events_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.POINTER(DetParams), _vp, _vp, C.c_int64]),
    # ... its device-resident form (all pointers device but params; the check against cap happens on the device)
    "sk_detect_events_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.POINTER(DetParams), _vp, _vp, C.c_int64]),
    # signal HMM ("signal HMM" in include/squigglekit_hip.h; tests/hmm_ref.py states it in numpy): sig, stride, len, nreads,
    # cal2 or NULL, model, limit, rec -- the device-resident form takes the same list
    "sk_hmm_viterbi_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.POINTER(HmmModel), C.c_int32, _vp]),
    "sk_hmm_viterbi_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.POINTER(HmmModel), C.c_int32, _vp]),
    # ... ragged float64 values: values, off, nreads, model, limit, rec
    "sk_hmm_viterbi_f64_len": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(HmmModel), C.c_int32, _vp]),
    # signal HMM state paths: the arguments of the matching sk_hmm_viterbi_* call, then off [nreads + 1], seg, cap
    "sk_hmm_segments_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.POINTER(HmmModel), C.c_int32, _vp, _vp, _vp,
                                      C.c_int64]),
    "sk_hmm_segments_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.POINTER(HmmModel), C.c_int32, _vp, _vp, _vp,
                                          C.c_int64]),
    "sk_hmm_segments_f64_len": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(HmmModel), C.c_int32, _vp, _vp, _vp, C.c_int64]),
    # signal HMM posteriors ("signal HMM: posteriors"; tests/hmm_post_ref.py states them in numpy): the arguments of the
    # matching sk_hmm_viterbi_* call with post in rec's place, then counts or NULL, then goff and gamma or both NULL
    "sk_hmm_posterior_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.POINTER(HmmModel), C.c_int32, _vp, _vp, _vp,
                                       _vp]),
    "sk_hmm_posterior_dev_i16": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, _vp, C.POINTER(HmmModel), C.c_int32, _vp, _vp,
                                           _vp, _vp]),
    "sk_hmm_posterior_f64_len": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(HmmModel), C.c_int32, _vp, _vp, _vp, _vp]),
    # MotifSeq sessions ("MotifSeq sessions" in include/squigglekit_hip.h; tests/stream_ref.py states them in numpy):
    # open(motifs, motif_off, nmotifs, params, handle); push(handle, slots, m, rows, stride, len, out [nmotifs][m]) and
    # its device-resident form; flush(handle, slots, m, out); reset(handle, slots, m, center, scale); close(handle)
    "sk_stream_open": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(StreamParams), _i32p]),
    "sk_stream_push_i16": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_int64, _vp, _vp]),
    "sk_stream_push_dev_i16": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_int64, _vp, _vp]),
    "sk_stream_flush": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp]),
    "sk_stream_reset": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, _vp]),
    "sk_stream_close": (C.c_int, [C.c_int32]),
    # mapping sessions ("Mapping sessions" in include/squigglekit_hip.h; tests/mapstream_ref.py states the chained rows):
    # open(targets, target_off, ntargets, nslots, handle); push(handle, slots, m, values, off, out [ntargets][m]) and its
    # device-resident form (off stays a host pointer); reset(handle, slots, m); close(handle); the last push's plan
    "sk_map_open": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _i32p]),
    "sk_map_push": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    "sk_map_push_dev": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    "sk_map_reset": (C.c_int, [C.c_int32, _vp, C.c_int32]),
    "sk_map_close": (C.c_int, [C.c_int32]),
    "sk_last_map_plan": (C.c_int, [_vp, _vp, _vp]),
    # hit lists over a pair list ("Hit lists over a pair list" in include/squigglekit_hip.h): the pair list, then max_hits,
    # max_dist, out [npairs][K], count [npairs]; from a session's stored rows: handle, slots, m, max_hits, max_dist, out
    # [T][m][K], count [T][m]; the last call's plan
    "sk_dtw_pairs_hits": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int64, C.c_int32, C.c_double, _vp, _vp]),
    "sk_dtw_pairs_hits_dev": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int64, C.c_int32, C.c_double, _vp, _vp]),
    "sk_map_hits": (C.c_int, [C.c_int32, _vp, C.c_int32, C.c_int32, C.c_double, _vp, _vp]),
    "sk_map_hits_dev": (C.c_int, [C.c_int32, _vp, C.c_int32, C.c_int32, C.c_double, _vp, _vp]),
    "sk_last_pair_hits_plan": (C.c_int, [_vp, _vp, _vp]),
    # event sessions ("Event sessions" in include/squigglekit_hip.h; tests/evstream_ref.py states them on detect_ref):
    # open(params, nslots, handle); push(handle, slots, m, rows, stride, len, end or NULL, off [m + 1], rec, cap) and its
    # device-resident form; fetch(handle, rec, cap); reset(handle, slots, m); close(handle); the last push's plan
    "sk_evs_open": (C.c_int, [C.POINTER(DetParams), C.c_int32, _i32p]),
    "sk_evs_push_i16": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_int64]),
    "sk_evs_push_dev_i16": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_int64]),
    "sk_evs_fetch": (C.c_int, [C.c_int32, _vp, C.c_int64]),
    "sk_evs_reset": (C.c_int, [C.c_int32, _vp, C.c_int32]),
    "sk_evs_close": (C.c_int, [C.c_int32]),
    "sk_last_evs_plan": (C.c_int, [_vp, _vp, _vp]),
    # HMM sessions ("HMM sessions" in include/squigglekit_hip.h; tests/hmmstream_ref.py states them on hmm_ref):
    # open(model, nslots, handle); push_i16(handle, slots, m, rows, stride, len, out [m]), push_f64(handle, slots, m,
    # values, off [m + 1], out [m]) and their device-resident forms; reset(handle, slots, m, cal2 or NULL);
    # close(handle); the last push's plan
    "sk_hmms_open": (C.c_int, [C.POINTER(HmmModel), C.c_int32, _i32p]),
    "sk_hmms_push_i16": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_int64, _vp, _vp]),
    "sk_hmms_push_dev_i16": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_int64, _vp, _vp]),
    "sk_hmms_push_f64": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    "sk_hmms_push_dev_f64": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    "sk_hmms_reset": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp]),
    "sk_hmms_close": (C.c_int, [C.c_int32]),
    "sk_last_hmms_plan": (C.c_int, [_vp, _vp]),
    # ... filtered sessions (SK_HMMS_FILTER): the forward recursion carried beside the Viterbi pass (tests/hmmfilter_ref.py)
    "sk_hmms_open_ex": (C.c_int, [C.POINTER(HmmModel), C.c_int32, C.c_int32, _i32p]),
    "sk_hmms_filter": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp]),
    "sk_hmms_filter_dev": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp]),
    # live mapping sessions ("Live mapping sessions" in include/squigglekit_hip.h; tests/live_ref.py states them on
    # evstream_ref and mapstream_ref): open(params, calib, targets, target_off, ntargets, nslots, handle); push(handle,
    # slots, m, rows, stride, len, end or NULL, rule or NULL, out [T][m], info [m], best [m] or NULL) and its
    # device-resident form; fetch(handle, off [m + 1], values, cap); hits as sk_map_hits; reset; close; the last plan
    "sk_live_open": (C.c_int, [C.POINTER(DetParams), C.c_int32, _vp, _vp, C.c_int32, C.c_int32, _i32p]),
    "sk_live_push_i16": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_int64, _vp, _vp, C.POINTER(LiveRule), _vp, _vp, _vp]),
    "sk_live_push_dev_i16": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_int64, _vp, _vp, C.POINTER(LiveRule), _vp, _vp,
                                       _vp]),
    "sk_live_fetch": (C.c_int, [C.c_int32, _vp, _vp, C.c_int64]),
    "sk_live_hits": (C.c_int, [C.c_int32, _vp, C.c_int32, C.c_int32, C.c_double, _vp, _vp]),
    "sk_live_reset": (C.c_int, [C.c_int32, _vp, C.c_int32]),
    "sk_live_close": (C.c_int, [C.c_int32]),
    "sk_last_live_plan": (C.c_int, [_vp, _vp, _vp]),
    "sk_live_last_ms": (C.c_int, [C.c_int32, _vp, _vp]),
    # gated live sessions ("Gated live sessions" in the header; tests/livegate_ref.py): open_gated(sk_live_open's
    # arguments up to nslots, model, gate, handle); reset_cal(handle, slots, m, cal2 [m][2]); gate_fetch(handle,
    # gate [m] or NULL, rec [m] or NULL) and its device-resident form
    "sk_live_open_gated": (C.c_int, [C.POINTER(DetParams), C.c_int32, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(HmmModel),
                                     C.POINTER(LiveGate), _i32p]),
    "sk_live_reset_cal": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp]),
    "sk_live_gate_fetch": (C.c_int, [C.c_int32, _vp, _vp]),
    "sk_live_gate_fetch_dev": (C.c_int, [C.c_int32, _vp, _vp]),
    "sk_live_gate_last_ms": (C.c_int, [C.c_int32, _vp, _vp]),
    # reference pile-up ("Reference pile-up" in the header; tests/pileup_ref.py states it in numpy): span_off, spans, value,
    # dwell, target, shift, use, npairs, nrows, tlen, ntargets, out [Mtot], ent_off, ent_row, ent_cap -- the device-resident
    # form takes the same list (tlen stays a host pointer); the last call's plan
    "sk_pileup": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp, C.c_int64]),
    "sk_pileup_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp,
                                C.c_int64]),
    "sk_last_pileup_plan": (C.c_int, [_vp, _vp, _vp, _vp]),
}


def build(force=False):
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-s", "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return SO_PATH


_lib = None


def load():
    """dlopen the library and bind every ABI symbol.  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise SquiggleKitError(-2, "%s not built (run `python -c 'import __graft_entry__ as g; "
                                   "g.build()'` or `make -C squigglekit_amd/csrc`); there is no CPU "
                                   "fallback" % SO_PATH)
        L = C.CDLL(SO_PATH)
        for name, (res, argt) in ABI.items():
            fn = getattr(L, name)            # AttributeError here == header/library drift
            fn.restype = res
            fn.argtypes = argt
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise SquiggleKitError(rc, load().sk_last_error().decode(errors="replace"))


_tls = threading.local()      # the library binds a device per host thread (thread_local in sk_runtime.hip)


def init(device=None, slot=None):
    """Bind the calling thread to a GPU (default: $SK_DEVICE, else LOCAL_RANK, else 0).  `slot`: an explicit
    context slot (sk_init_slot) -- several threads sharing one GPU each need their own."""
    L = load()
    if device is None:
        device = int(os.environ.get("SK_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    if slot is None:
        check(L.sk_init(int(device)))
    else:
        check(L.sk_init_slot(int(slot), int(device)))
    _tls.device = int(device)
    _ready.set()
    return _tls.device


_ready = threading.Event()


def is_ready():
    """Has some thread of this process already bound a GPU (so that init() costs nothing now)?"""
    return _ready.is_set()


def warm_start(device=None, also=()):
    """Start binding the GPU on a background thread (the HIP runtime's start-up costs a few hundred milliseconds that a
    command-line tool can spend parsing its first chunk of input) and import the modules named in `also` there too.
    Every thread binds for itself later (init / ensure_init), by then at no cost.  Returns the thread."""
    if device is not None:
        os.environ["SK_DEVICE"] = str(int(device))

    def run():
        try:
            init(device)
            for mod in also:
                __import__(mod)
        except Exception:                                            # noqa: BLE001 -- the foreground call reports it
            pass
    t = threading.Thread(target=run, name="sk-warm", daemon=True)
    t.start()
    return t


def ensure_init():
    if getattr(_tls, "device", None) is None:
        init()
    return load()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# Host-side tuning switches (the native ones live in csrc/sk_runtime.hip: SK_TUNABLES): name -> (values the parity
# test flips it to, description).  Like the native ones they are read only when SK_TUNING=1 is set as well.
PY_TUNABLES = {
    "SK_BLOW5_PIN": ("1", "BLOW5 reader: page-locked streaming buffers"),
    "SK_BLOW5_BLOCK": ("64 5000", "BLOW5 reader: records per block"),
    "SK_BLOW5_ZAP": ("0", "BLOW5 reader: keep the consumed pages of the file map"),
    "SK_I16_PIN": ("1", "--i16 reader: page-locked streaming buffers"),
    "SK_I16_BLOCK_MB": ("1 8", "--i16 reader: block size in MB"),
    "SK_TSV_THREADS": ("4 64", "TSV reader: worker threads of the native tokenizer (default 32)"),
    "SK_TSV_NO_CENTI": ("1", "TSV reader: decimal lines through the float64 tokenizer even when every token has at most two decimals"),
}


def tune(name, default=None):
    """Value of a host-side tuning switch, or `default` when it is unset or SK_TUNING=1 is not set."""
    if os.environ.get("SK_TUNING", "")[:1] != "1" or name not in PY_TUNABLES:
        return default
    return os.environ.get(name, default)


def tunables():
    """Every tuning switch: {name: (test values, description)} -- the native table plus PY_TUNABLES."""
    L = load()
    n = L.sk_tunables(None, 0)
    buf = C.create_string_buffer(n)
    L.sk_tunables(buf, n)
    out = {}
    for line in buf.value.decode().splitlines():
        name, vals, what = line.split("\t")
        out[name] = (vals, what)
    out.update(PY_TUNABLES)
    return out
