"""ctypes mirror of include/sdhip.h -- the host-side binding the tests, bench.py and
__graft_entry__ use.  It only loads libsdhip.so (built in-tree next to this file) and
fails loudly when the library or the GPU is missing: there is no CPU fallback.

Names follow the reference's operator seams: segment ~ SegmentModel::slide,
embed ~ getEmbedding + EmbeddingModel1::infer, cluster ~ Clustering::cluster,
diarize ~ speakerDiarization()."""
import ctypes as C
import math
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDHIP_LIB") or os.path.join(_HERE, "libsdhip.so")      # (SDHIP_LIB: instrumented builds of the tuning tools)

CHUNK, HOP, FRAMES, SPEAKERS, EMB_DIM, EMB_BATCH = 80000, 8000, 293, 3, 192, 32
T_FRAMES, N_MELS = 501, 80


class Turn(C.Structure):
    _fields_ = [("start", C.c_double), ("end", C.c_double), ("label", C.c_int32), ("_pad", C.c_int32)]


class DerResult(C.Structure):
    """sd_der_result of include/sdhip.h"""
    _fields_ = [(n, C.c_double) for n in ("der", "total", "missed", "false_alarm", "confusion", "correct")]


class CutSpec(C.Structure):
    """sd_cut_spec of include/sdhip.h"""
    _fields_ = [("threshold", C.c_double), ("min_cluster_size", C.c_int32), ("num_clusters", C.c_int32)]


class ConvCase(C.Structure):
    """sd_conv_case of include/sdhip_test.h"""
    _fields_ = [(n, C.c_int32) for n in (
        "items", "dense", "tin", "t", "tp_in", "tp_out", "cin", "cin_pad", "cout", "kt", "dil", "pad_mode",
        "shared", "x_ld", "x_col0", "has_x2", "x2_col0", "y_ld", "y_col0", "y_f32", "act1", "act2", "prec", "try_narrow")] + [("canary", C.c_float)]


CONV_SLACK_ROWS = 256      # guard rows behind the buffers of Diarizer.conv_case
SEG_SLACK_ROWS = 256       # ... and behind those of Diarizer.lstm_rec_case / pool_norm_case / chunk_norm_case / classifier_case
GLUE_SLACK_ROWS = 256      # ... and behind those of Diarizer.ecapa_stats_case / se_apply_case / scatter_emb_case / to_half_case
ROWTAB_SLACK = 128         # slack entries behind the table of Diarizer.rowtab_case
BE_SLACK = 256             # slack units behind every array of the Diarizer.*_case methods of the back end (binarize_case .. mark_inactive_case)
BE_BCANARY = 0xA5          # SD_TEST_BCANARY: what their byte outputs are preset to
IN_SLACK = 256             # slack elements behind every array of Diarizer.resample_case .. weight_forms_case
FE_SLACK = 256            # slack entries (feature rows) behind every array of Diarizer.frontend_prepare_case / frontend_features_case / frontend_signals_case


ENC_S16, ENC_F32, ENC_MULAW, ENC_ALAW = 0, 1, 2, 3      # SD_ENC_*
_ENC_DTYPES = {ENC_S16: np.int16, ENC_F32: np.float32, ENC_MULAW: np.uint8, ENC_ALAW: np.uint8}


class AudioDesc(C.Structure):
    """sd_audio"""
    _fields_ = [("data", C.c_void_p), ("n", C.c_int64), ("sample_rate", C.c_int32), ("encoding", C.c_int32), ("channels", C.c_int32), ("channel", C.c_int32)]


class Audio:
    """One recording of Diarizer.diarize_many_audio (sd_audio): data = the interleaved elements as they arrive -- int16 (ENC_S16), float32 (ENC_F32) or
    one G.711 code per uint8 (ENC_MULAW / ENC_ALAW) --, n frames of `channels` elements at sample_rate Hz; channel = the one to take, -1 = the mean of all.
    For diarize_many_audio_dev data is a device pointer (an int) and n must be given."""

    def __init__(self, data, sample_rate=16000, encoding=ENC_S16, channels=1, channel=0, n=None):
        self.sample_rate, self.encoding, self.channels, self.channel = int(sample_rate), int(encoding), int(channels), int(channel)
        if isinstance(data, (int, np.integer)):
            self.data, self.ptr, self.n = None, int(data), int(n)
        else:
            self.data = np.ascontiguousarray(data, _ENC_DTYPES.get(self.encoding, np.uint8)).reshape(-1)
            self.n = len(self.data) // max(self.channels, 1) if n is None else int(n)
            self.ptr = self.data.ctypes.data if self.data.size else 0

    def desc(self):
        return AudioDesc(self.ptr or None, self.n, self.sample_rate, self.encoding, self.channels, self.channel)


class SdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libsdhip error %d: %s" % (code, msg))
        self.code = code


_lib = None

# every symbol include/sdhip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "sd_create", "sd_destroy", "sd_last_error", "sd_create_error", "sd_num_chunks", "sd_segment", "sd_segment_dev",
    "sd_postseg", "sd_count_frames", "sd_embed", "sd_embed_dev", "sd_frontend", "sd_ecapa", "sd_linkage", "sd_cluster",
    "sd_clustering", "sd_clustering_ex", "sd_reconstruct", "sd_diarize", "sd_diarize_dev", "sd_free_turns", "sd_shard_infer_dev",
    "sd_finalize_dev", "sd_read_wav", "sd_free_pcm", "sd_format_turn", "sd_stage_ms", "sd_kernel_stats",
    "sd_reset_stats", "sd_set_option", "sd_bench_conv", "sd_convert_onnx", "sd_convert_error", "sd_read_wav_f32", "sd_free_wav", "sd_diarize_f32",
    "sd_write_rttm", "sd_set_planted", "sd_comm_unique_id", "sd_comm_init", "sd_comm_destroy", "sd_comm_info", "sd_shard_plan",
    "sd_diarize_sharded", "sd_diarize_sharded_dev", "sd_write_rttm_ex", "sd_relabel_turns", "sd_relabel_turns_ex", "sd_last_confidence",
    "sd_debug_read_ws", "sd_test_pack_split_weights", "sd_resample", "sd_resample_len", "sd_diarize_wav", "sd_set_dump_dir",
    "sd_fcluster", "sd_segment_chunks", "sd_embed_signals",
    "sd_linkage_ex", "sd_cluster_ex", "sd_set_option_f64", "sd_linkage_method_from_name", "sd_test_conv", "sd_test_emb_batches",
    "sd_test_lstm_rec", "sd_test_pool_norm", "sd_test_chunk_norm", "sd_test_classifier",
    "sd_test_ecapa_stats", "sd_test_se_apply", "sd_test_rowtab", "sd_test_scatter_emb", "sd_test_to_half",
    "sd_test_frontend_prepare", "sd_test_frontend_features", "sd_test_frontend_signals",
    "sd_test_binarize", "sd_test_count", "sd_test_gather_normalize", "sd_test_cluster_means", "sd_test_assign", "sd_test_constrained_argmax",
    "sd_test_activations", "sd_test_topk", "sd_test_assign_cuts", "sd_test_recon_cuts", "sd_test_pcm_to_f32", "sd_test_f32_to_f64", "sd_test_mark_inactive",
    "sd_test_resample", "sd_test_resample_jobs", "sd_test_group_copy", "sd_test_many_pack", "sd_test_many_gap_masks", "sd_test_weight_forms",
    "sd_activity_scores", "sd_activity_regions", "sd_activity", "sd_activity_dev", "sd_activity_f32", "sd_activity_wav", "sd_last_activity_scores",
    "sd_stream_open", "sd_stream_push", "sd_stream_push_dev", "sd_stream_push_f32", "sd_stream_turns", "sd_stream_info", "sd_stream_read",
    "sd_stream_close", "sd_stream_sealed_chunks", "sd_stream_forget", "sd_stream_set_window", "sd_stream_origin",
    "sd_stream_push_many", "sd_stream_push_many_dev", "sd_stream_push_many_f32", "sd_stream_turns_many",
    "sd_last_speakers", "sd_span_masks", "sd_voiceprint", "sd_voiceprint_dev", "sd_voiceprint_f32", "sd_voiceprint_wav", "sd_speaker_distances",
    "sd_match_speakers", "sd_read_voiceprints", "sd_write_voiceprints", "sd_free_voiceprints", "sd_voiceprints_error", "sd_write_rttm_named",
    "sd_set_enrolled", "sd_enrolled_info", "sd_nearest_speakers", "sd_last_enrolled",
    "sd_many_plan", "sd_diarize_many", "sd_diarize_many_dev", "sd_diarize_many_f32", "sd_many_select",
    "sd_der", "sd_read_rttm", "sd_free_rttm_names", "sd_score_error",
    "sd_cut_open_dev", "sd_cut_open", "sd_cut_open_pcm_dev", "sd_cut_open_f32", "sd_cut_open_wav", "sd_cut_turns", "sd_cut_turns_many",
    "sd_cut_dendrogram", "sd_cut_info", "sd_cut_close",
    "sd_sample_rows",
    "sd_roster_open", "sd_roster_close", "sd_roster_load", "sd_roster_info", "sd_roster_speakers", "sd_roster_update", "sd_roster_update_last",
    "sd_relabel_turns_map", "sd_stream_set_roster", "sd_last_roster_ids",
    "sd_linkage_many",
    "sd_stream_set_input_rate", "sd_stream_end_input", "sd_stream_input_info", "sd_resample_final_len",
    "sd_audio_len16", "sd_g711_decode", "sd_read_wav_audio", "sd_diarize_many_audio", "sd_diarize_many_audio_dev",
    "sd_stream_set_input_format", "sd_stream_input_format", "sd_stream_push_audio", "sd_stream_push_audio_dev",
    "sd_stream_push_many_audio", "sd_stream_push_many_audio_dev",
]
# the stream hook of include/sdhip_stream_test.h (sdhip_test.h's list is pinned name by name by tests/test_abi.py)
STREAM_TEST_EXPORTS = ["sd_test_stream_tail"]
# the hook of k_many_ingest, include/sdhip_ingest_test.h (likewise)
INGEST_TEST_EXPORTS = ["sd_test_many_ingest"]
# the hook of k_group_ingest, include/sdhip_stream_ingest_test.h (likewise)
STREAM_INGEST_TEST_EXPORTS = ["sd_test_group_ingest"]
# SD_LINKAGE_* (scipy's method codes) and SD_METRIC_*
LINKAGE_METHODS = ("single", "complete", "average", "centroid", "median", "ward", "weighted")
METRIC_EUCLIDEAN, METRIC_COSINE = 0, 1
CLUSTERING_THRESHOLD_DEFAULT = float(np.float32(0.7153814381597874))      # the reference's float constant, widened (sd.cpp:2049)
COMM_ID_BYTES = 128
ACTIVITY_SPEECH, ACTIVITY_OVERLAP = 0, 1      # SD_ACTIVITY_*
ACTIVITY_KINDS = ("speech", "overlap")
SPEAKER_MATCH_THRESHOLD_DEFAULT = CLUSTERING_THRESHOLD_DEFAULT * CLUSTERING_THRESHOLD_DEFAULT / 2      # option "speaker_match_threshold": t * t / 2


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libsdhip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(or make -C '%s')" % _HERE)
    L = C.CDLL(LIB_PATH)
    vp, i64, i32, dbl = C.c_void_p, C.c_int64, C.c_int32, C.c_double
    L.sd_create.restype = vp
    L.sd_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.sd_destroy.argtypes = [vp]
    L.sd_last_error.restype = C.c_char_p
    L.sd_last_error.argtypes = [vp]
    L.sd_create_error.restype = C.c_char_p
    L.sd_num_chunks.restype = i64
    L.sd_num_chunks.argtypes = [i64, C.POINTER(i64)]
    L.sd_count_frames.restype = i64
    L.sd_count_frames.argtypes = [i64]
    L.sd_set_dump_dir.argtypes = [vp, C.c_char_p, C.c_int]
    L.sd_resample_len.restype = i64
    L.sd_resample_len.argtypes = [i64, i32, i32]
    L.sd_resample.argtypes = [vp, vp, i64, i32, i32, vp, i64, C.POINTER(i64)]
    L.sd_diarize_wav.argtypes = [vp, C.c_char_p, C.c_int, C.POINTER(C.POINTER(Turn)), C.POINTER(i64)]
    L.sd_segment.argtypes = [vp, vp, i64, vp, C.POINTER(i64)]
    L.sd_segment_dev.argtypes = [vp, vp, i64, vp, i64]
    L.sd_postseg.argtypes = [vp, vp, i64, vp, vp, vp, i64, C.POINTER(i64)]
    L.sd_embed.argtypes = [vp, vp, i64, vp, i64, vp]
    L.sd_embed_dev.argtypes = [vp, vp, i64, vp, i64, i64, vp]
    L.sd_frontend.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    L.sd_ecapa.argtypes = [vp, vp, vp, i64, vp]
    L.sd_linkage.argtypes = [vp, vp, i64, C.c_int, vp]
    L.sd_fcluster.argtypes = [vp, vp, i64, dbl, vp]
    L.sd_segment_chunks.argtypes = [vp, vp, i64, i64, vp, C.POINTER(i32)]
    L.sd_embed_signals.argtypes = [vp, vp, vp, i64, vp]
    L.sd_cluster.argtypes = [vp, vp, i64, C.c_int, dbl, vp]
    L.sd_linkage_ex.argtypes = [vp, vp, i64, C.c_int, C.c_int, C.c_int, vp]
    L.sd_cluster_ex.argtypes = [vp, vp, i64, C.c_int, C.c_int, C.c_int, dbl, vp]
    L.sd_linkage_many.argtypes = [vp, vp, vp, i64, C.c_int, C.c_int, C.c_int, vp, vp]
    L.sd_set_option_f64.argtypes = [vp, C.c_char_p, dbl]
    L.sd_linkage_method_from_name.argtypes = [C.c_char_p]
    L.sd_clustering.argtypes = [vp, vp, i64, C.c_int, vp, C.POINTER(i32)]
    L.sd_clustering_ex.argtypes = [vp, vp, i64, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(i32)]
    L.sd_reconstruct.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, C.POINTER(C.POINTER(Turn)), C.POINTER(i64)]
    L.sd_diarize.argtypes = [vp, vp, i64, C.POINTER(C.POINTER(Turn)), C.POINTER(i64)]
    L.sd_diarize_dev.argtypes = [vp, vp, i64, C.POINTER(C.POINTER(Turn)), C.POINTER(i64)]
    L.sd_free_turns.argtypes = [C.POINTER(Turn)]
    L.sd_shard_infer_dev.argtypes = [vp, vp, i64, i64, i64, i64, i64, vp, vp]
    L.sd_finalize_dev.argtypes = [vp, vp, vp, i64, i64, C.POINTER(C.POINTER(Turn)), C.POINTER(i64)]
    L.sd_read_wav.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_int16)), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)]
    L.sd_free_pcm.argtypes = [C.POINTER(C.c_int16)]
    L.sd_read_wav_f32.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.sd_free_wav.argtypes = [C.POINTER(C.c_float)]
    L.sd_diarize_f32.argtypes = [vp, vp, i64, C.POINTER(C.POINTER(Turn)), C.POINTER(i64)]
    L.sd_write_rttm.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Turn), i64]
    L.sd_set_planted.argtypes = [vp, vp, vp, i64, i64]
    L.sd_comm_unique_id.argtypes = [vp]
    L.sd_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
    L.sd_comm_destroy.argtypes = [vp]
    L.sd_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.sd_shard_plan.argtypes = [i64, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    L.sd_diarize_sharded.argtypes = [vp, vp, i64, i64, i64, C.POINTER(C.POINTER(Turn)), C.POINTER(i64)]
    L.sd_diarize_sharded_dev.argtypes = [vp, vp, i64, i64, i64, C.POINTER(C.POINTER(Turn)), C.POINTER(i64)]
    L.sd_write_rttm_ex.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Turn), i64, C.POINTER(dbl)]
    L.sd_relabel_turns.argtypes = [C.POINTER(Turn), i64]
    L.sd_relabel_turns_ex.argtypes = [C.POINTER(Turn), i64, C.c_int]
    L.sd_last_confidence.argtypes = [vp, C.POINTER(dbl), i64, C.POINTER(i64)]
    tpp = C.POINTER(C.POINTER(Turn))
    L.sd_activity_scores.argtypes = [vp, vp, i64, C.c_int, vp, i64, C.POINTER(i64)]
    L.sd_activity_regions.argtypes = [vp, vp, i64, tpp, C.POINTER(i64)]
    L.sd_activity.argtypes = [vp, vp, i64, C.c_int, tpp, C.POINTER(i64)]
    L.sd_activity_dev.argtypes = [vp, vp, i64, C.c_int, tpp, C.POINTER(i64)]
    L.sd_activity_f32.argtypes = [vp, vp, i64, C.c_int, tpp, C.POINTER(i64)]
    L.sd_activity_wav.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, tpp, C.POINTER(i64)]
    L.sd_last_activity_scores.argtypes = [vp, C.POINTER(dbl), i64, C.POINTER(i64)]
    L.sd_stream_open.argtypes = [vp, C.POINTER(vp)]
    L.sd_stream_push.argtypes = [vp, vp, i64]
    L.sd_stream_push_dev.argtypes = [vp, vp, i64]
    L.sd_stream_push_f32.argtypes = [vp, vp, i64]
    L.sd_stream_turns.argtypes = [vp, tpp, C.POINTER(i64)]
    L.sd_stream_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.sd_stream_read.argtypes = [vp, i64, i64, vp, vp]
    L.sd_stream_close.argtypes = [vp]
    L.sd_stream_close.restype = None
    L.sd_stream_sealed_chunks.restype = i64
    L.sd_stream_sealed_chunks.argtypes = [i64]
    L.sd_last_speakers.argtypes = [vp, vp, i64, C.POINTER(i64), vp]
    L.sd_span_masks.argtypes = [vp, i64, vp, i64, i32, vp]
    L.sd_voiceprint.argtypes = [vp, vp, i64, vp, i64, i32, vp, C.POINTER(i64)]
    L.sd_voiceprint_dev.argtypes = [vp, vp, i64, vp, i64, i32, vp, C.POINTER(i64)]
    L.sd_voiceprint_f32.argtypes = [vp, vp, i64, vp, i64, i32, vp, C.POINTER(i64)]
    L.sd_voiceprint_wav.argtypes = [vp, C.c_char_p, C.c_int, vp, i64, i32, vp, C.POINTER(i64)]
    L.sd_speaker_distances.argtypes = [vp, vp, i64, vp, i64, C.c_int, vp]
    L.sd_match_speakers.argtypes = [vp, vp, i64, vp, i64, C.c_int, dbl, vp, vp]
    L.sd_read_voiceprints.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(dbl)), C.POINTER(i64)]
    L.sd_write_voiceprints.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), vp, i64]
    L.sd_free_voiceprints.argtypes = [C.POINTER(C.c_char_p), C.POINTER(dbl), i64]
    L.sd_free_voiceprints.restype = None
    L.sd_voiceprints_error.restype = C.c_char_p
    L.sd_write_rttm_named.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Turn), i64, C.POINTER(dbl), C.POINTER(C.c_char_p), i64]
    L.sd_set_enrolled.argtypes = [vp, vp, i64, C.c_int]
    L.sd_enrolled_info.argtypes = [vp, C.POINTER(i64), C.POINTER(C.c_int)]
    L.sd_nearest_speakers.argtypes = [vp, vp, i64, vp, i64, C.c_int, vp, vp]
    L.sd_last_enrolled.argtypes = [vp, vp, i64, C.POINTER(i64)]
    if hasattr(L, "sd_many_plan"):      # (an older build loaded through SDHIP_LIB by the A/B tools has none of these)
        L.sd_many_plan.argtypes = [vp, i64, vp, vp]
        for f in (L.sd_diarize_many, L.sd_diarize_many_dev, L.sd_diarize_many_f32):
            f.argtypes = [vp, vp, vp, i64, vp, vp, vp]
        L.sd_many_select.argtypes = [vp, i64]
    if hasattr(L, "sd_stream_push_many"):      # (likewise)
        for f in (L.sd_stream_push_many, L.sd_stream_push_many_dev, L.sd_stream_push_many_f32):
            f.argtypes = [vp, vp, vp, i64]
        L.sd_stream_turns_many.argtypes = [vp, i64, vp, vp, vp]
    if hasattr(L, "sd_der"):           # (an older build loaded through SDHIP_LIB by the A/B tools has none of these)
        L.sd_der.argtypes = [C.POINTER(Turn), i64, C.POINTER(Turn), i64, C.POINTER(Turn), i64, dbl, C.c_int, C.POINTER(DerResult), vp, i64, C.POINTER(i64)]
        L.sd_read_rttm.argtypes = [C.c_char_p, C.c_char_p, tpp, C.POINTER(i64), C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(i64)]
        L.sd_free_rttm_names.argtypes = [C.POINTER(C.c_char_p), i64]
        L.sd_free_rttm_names.restype = None
        L.sd_score_error.restype = C.c_char_p
        L.sd_cut_open_dev.argtypes = [vp, vp, vp, i64, i64, C.POINTER(vp)]
        for f in (L.sd_cut_open, L.sd_cut_open_pcm_dev, L.sd_cut_open_f32):
            f.argtypes = [vp, vp, i64, C.POINTER(vp)]
        L.sd_cut_open_wav.argtypes = [vp, C.c_char_p, C.c_int, C.POINTER(vp)]
        L.sd_cut_turns.argtypes = [vp, C.POINTER(CutSpec), tpp, C.POINTER(i64), C.POINTER(i32)]
        L.sd_cut_turns_many.argtypes = [vp, C.POINTER(CutSpec), i64, tpp, C.POINTER(i64), C.POINTER(i32)]
        L.sd_cut_dendrogram.argtypes = [vp, vp, i64, C.POINTER(i64)]
        L.sd_cut_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        L.sd_cut_close.argtypes = [vp]
        L.sd_cut_close.restype = None
    if hasattr(L, "sd_sample_rows"):      # (likewise)
        L.sd_sample_rows.restype = i64
        L.sd_sample_rows.argtypes = [vp, i64, i64, i64, vp]
        L.sd_stream_forget.argtypes = [vp, i64]
        L.sd_stream_set_window.argtypes = [vp, i64]
        L.sd_stream_origin.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "sd_roster_open"):      # (likewise)
        L.sd_roster_open.argtypes = [C.c_int, C.POINTER(vp)]
        L.sd_roster_close.argtypes = [vp]
        L.sd_roster_load.argtypes = [vp, vp, vp, i64]
        L.sd_roster_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int)]
        L.sd_roster_speakers.argtypes = [vp, vp, vp, vp, i64, C.POINTER(i64)]
        L.sd_roster_update.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64, i64, dbl, vp]
        L.sd_roster_update_last.argtypes = [vp, vp, vp, i64, C.POINTER(i64)]
        L.sd_relabel_turns_map.argtypes = [C.POINTER(Turn), i64, vp, i64]
        L.sd_stream_set_roster.argtypes = [vp, vp]
        L.sd_last_roster_ids.argtypes = [vp, vp, i64, C.POINTER(i64)]
    if hasattr(L, "sd_stream_set_input_rate"):      # (likewise)
        L.sd_stream_set_input_rate.argtypes = [vp, i32]
        L.sd_stream_end_input.argtypes = [vp]
        L.sd_stream_input_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]
        L.sd_resample_final_len.restype = i64
        L.sd_resample_final_len.argtypes = [i64, i32, i32]
        L.sd_test_stream_tail.argtypes = [vp, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    if hasattr(L, "sd_diarize_many_audio"):      # (likewise)
        L.sd_audio_len16.restype = i64
        L.sd_audio_len16.argtypes = [C.POINTER(AudioDesc)]
        L.sd_g711_decode.argtypes = [i32, vp, i64, vp]
        L.sd_read_wav_audio.argtypes = [C.c_char_p, C.POINTER(AudioDesc), C.POINTER(vp)]
        for f in (L.sd_diarize_many_audio, L.sd_diarize_many_audio_dev):
            f.argtypes = [vp, C.POINTER(AudioDesc), i64, vp, vp, vp]
        L.sd_test_many_ingest.argtypes = [vp, vp, i64, vp, i64, i64, C.c_float, vp]
    if hasattr(L, "sd_stream_set_input_format"):      # (likewise)
        L.sd_stream_set_input_format.argtypes = [vp, i32, i32, i32]
        L.sd_stream_input_format.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
        for f in (L.sd_stream_push_audio, L.sd_stream_push_audio_dev):
            f.argtypes = [vp, vp, i64]
        for f in (L.sd_stream_push_many_audio, L.sd_stream_push_many_audio_dev):
            f.argtypes = [vp, vp, vp, i64]
        L.sd_test_group_ingest.argtypes = [vp, vp, i64, vp, i64, i64, C.c_float, vp]
    L.sd_format_turn.argtypes = [C.POINTER(Turn), C.c_char_p, C.c_int]
    L.sd_stage_ms.argtypes = [vp, C.POINTER(dbl)]
    L.sd_kernel_stats.argtypes = [vp, C.c_char_p, C.POINTER(dbl), C.POINTER(i64), C.POINTER(dbl), C.POINTER(dbl)]
    L.sd_reset_stats.argtypes = [vp]
    L.sd_set_option.argtypes = [vp, C.c_char_p, i64]
    L.sd_convert_onnx.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
    L.sd_convert_error.restype = C.c_char_p
    L.sd_debug_read_ws.argtypes = [vp, C.c_char_p, i64, vp, i64]
    L.sd_test_pack_split_weights.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.sd_bench_conv.argtypes = [vp, i64] + [C.c_int] * 9 + [C.POINTER(dbl)]
    L.sd_test_conv.argtypes = [vp, C.POINTER(ConvCase)] + [vp] * 10 + [C.c_char_p, C.c_int]
    L.sd_test_lstm_rec.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.c_int, C.c_float, vp]
    L.sd_test_pool_norm.argtypes = [vp, vp, i64, i64, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_float, vp]
    L.sd_test_chunk_norm.argtypes = [vp, vp, i64, i64, i64, i64, C.c_int, i64, C.c_float, C.c_float, C.c_int, C.c_float, vp]
    L.sd_test_classifier.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.c_float, vp]
    L.sd_test_ecapa_stats.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, i64, C.c_int, C.c_int, C.c_int, C.c_float, vp]
    L.sd_test_se_apply.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp] + [C.c_int] * 5 + [vp, i64, C.c_int, C.c_int, C.c_int, C.c_float, vp]
    L.sd_test_rowtab.argtypes = [vp, vp, vp, i64, i32, vp]
    L.sd_test_scatter_emb.argtypes = [vp, vp, i64, vp, i64, C.c_float, vp]
    L.sd_test_to_half.argtypes = [vp, C.c_int, vp, i64, C.c_int, C.c_float, vp]
    L.sd_test_frontend_prepare.argtypes = [vp, vp, i64, i64, C.c_int, i32, C.c_float] + [vp] * 11
    L.sd_test_frontend_features.argtypes = [vp, vp, i64, i64, i64, i64, vp, i64, C.c_int, C.c_float, vp, i64, vp, vp, vp]
    L.sd_test_frontend_signals.argtypes = [vp, vp, vp, i64, C.c_int, i32, C.c_float, vp, vp, vp, i64, vp, vp]
    L.sd_test_binarize.argtypes = [vp, vp, i64, C.c_float, i32, vp, vp, vp]
    L.sd_test_count.argtypes = [vp, vp, i64, C.c_float, i32, vp, vp]
    L.sd_test_gather_normalize.argtypes = [vp, vp, i64, vp, i64, C.c_int, C.c_float, vp, vp]
    L.sd_test_cluster_means.argtypes = [vp, vp, i64, C.c_int, vp, vp, C.c_int, C.c_float, vp]
    L.sd_test_assign.argtypes = [vp, vp, i64, C.c_int, vp, C.c_int, C.c_float, i32, vp, vp, vp, vp]
    L.sd_test_constrained_argmax.argtypes = [vp, vp, i64, C.c_int, dbl, i32, vp]
    L.sd_test_activations.argtypes = [vp, vp, vp, i64, C.c_int, C.c_float, vp, i64, vp]
    L.sd_test_topk.argtypes = [vp, vp, i64, vp, i64, i64, i64, i64, i64, C.c_int, vp]
    L.sd_test_assign_cuts.argtypes = [vp, vp, i64, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, C.c_float, i32, vp, vp, vp, vp]
    L.sd_test_recon_cuts.argtypes = [vp, vp, vp, i64, vp, C.c_int, vp, vp, i64, i64, i64, i64, i64, C.c_float, vp, i64, vp, vp]
    L.sd_test_pcm_to_f32.argtypes = [vp, vp, i64, C.c_float, vp]
    L.sd_test_f32_to_f64.argtypes = [vp, vp, i64, C.c_float, vp]
    L.sd_test_mark_inactive.argtypes = [vp, vp, vp, i64, i32, vp]
    L.sd_test_resample.argtypes = [vp, vp, i64, i32, i32, i64, C.c_float, vp, vp, i64]
    L.sd_test_resample_jobs.argtypes = [vp, vp, i64, vp, i64, i64, C.c_float, vp]
    L.sd_test_group_copy.argtypes = [vp, C.c_int, C.c_int, vp, i64, vp, i64, i64, C.c_float, vp]
    L.sd_test_many_pack.argtypes = [vp, C.c_int, vp, i64, vp, i64, i64, C.c_float, vp]
    L.sd_test_many_gap_masks.argtypes = [vp, vp, i64, i64, C.c_float, vp]
    L.sd_test_weight_forms.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint16, vp, i64, vp]
    L.sd_test_emb_batches.restype = i64
    L.sd_test_emb_batches.argtypes = [vp, i64, i64, C.c_int, C.c_int, vp, i64]
    _lib = L
    return L


def resample_final_len(n, in_sr, out_sr=16000):
    """sd_resample_final_len: F(n), the outputs of n inputs at in_sr that no later input can change (include/sdhip.h, "streams at any sample rate");
    -1 on bad arguments.  Host-only."""
    return int(lib().sd_resample_final_len(int(n), int(in_sr), int(out_sr)))


def linkage_method_from_name(name):
    """sd_linkage_method_from_name: scipy's method code of a linkage name, -1 for an unknown one.  Host-only."""
    return int(lib().sd_linkage_method_from_name(str(name).encode()))


def _activity_kind(kind):
    """'speech' / 'overlap' or SD_ACTIVITY_* -> the code (an unknown name -> -1, which the library refuses)"""
    if isinstance(kind, (int, np.integer)):
        return int(kind)
    return ACTIVITY_KINDS.index(kind) if kind in ACTIVITY_KINDS else -1


def _method_code(method):
    code = method if isinstance(method, (int, np.integer)) else linkage_method_from_name(method)
    return int(code)


def num_chunks(n):
    ll = C.c_int64(0)
    c = lib().sd_num_chunks(n, C.byref(ll))
    return int(c), int(ll.value)


def sealed_chunks(n):
    """sd_stream_sealed_chunks: chunks of an n-sample recording whose scores and embeddings are final, 32 * (full / 32).  Host-only."""
    return int(lib().sd_stream_sealed_chunks(int(n)))


def fcluster(Z, cutoff):
    """sd_fcluster = Clustering::fcluster (clustering.h:9-10): Z [N-1][4] -> 1-based labels [N].  Host arithmetic, no context, no GPU."""
    Z = np.ascontiguousarray(Z, np.float64).reshape(-1, 4)
    N = len(Z) + 1
    T = np.zeros(N, np.int32)
    rc = lib().sd_fcluster(None, _ptr(Z) if len(Z) else None, N, float(cutoff), _ptr(T))
    if rc:
        raise SdError(rc, "sd_fcluster: Z is not a dendrogram")
    return T


def emb_batches(nvalid, batch_items=3072, skip_dead_rows=True, balance=False):
    """sd_test_emb_batches: end index of every batch the embedding stage forms for items of `nvalid` valid frames.  Host-only, no context."""
    nv = np.ascontiguousarray(nvalid, np.int32)
    bounds = np.zeros(max(len(nv), 1), np.int64)
    nb = lib().sd_test_emb_batches(_ptr(nv), len(nv), int(batch_items), int(bool(skip_dead_rows)), int(bool(balance)), _ptr(bounds), len(bounds))
    if nb < 0:
        raise SdError(-nb, "sd_test_emb_batches: bad argument")
    return [int(b) for b in bounds[:nb]]


def shard_plan(n_total, world, rank0_permille=-1):
    """sd_shard_plan: (slot size in chunks of the padded all-gather, [(lo, hi)] by rank) -- contiguous chunk ranges, each
    starting on a multiple of 32 chunks (= 96 items = 3 reference embedding batches)"""
    arr = (C.c_int64 * (2 * world))()
    per = C.c_int64(0)
    rc = lib().sd_shard_plan(n_total, world, rank0_permille, arr, C.byref(per))
    if rc:
        raise SdError(rc, "sd_shard_plan: bad argument")
    return int(per.value), [(int(arr[2 * r]), int(arr[2 * r + 1])) for r in range(world)]


def plan_shards(n_total, world):
    """equal shares"""
    return shard_plan(n_total, world, -1)


def plan_ranks(n_total, world, rank0_fraction=None):
    """chunk range of every rank when rank 0, which also finalizes (count / clustering / reconstruction), is given a
    smaller share of the chunks: rank0_fraction of all chunks (0 = none), the other ranks split the rest evenly.
    None = equal shares.  Returns (per, [(lo, hi)] by rank): per = slot size of the padded all-gather."""
    if rank0_fraction is None or world == 1:
        return shard_plan(n_total, world, -1)
    return shard_plan(n_total, world, int(round(1000.0 * max(0.0, min(1.0, rank0_fraction)))))


def gather_pieces(per, ranges):
    """[(offset in the gathered buffer, chunks)] in chunk order: what rank 0 concatenates before finalizing"""
    return [(r * per, hi - lo) for r, (lo, hi) in enumerate(ranges) if hi > lo]


def shard_sample_range(lo, hi, n_total):
    """samples a rank must hold for chunks [lo, hi): [lo*8000, min(n, (hi-1)*8000 + 80000))"""
    if hi <= lo:
        return lo * HOP, lo * HOP
    return lo * HOP, min(n_total, (hi - 1) * HOP + CHUNK)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def many_plan(lengths):
    """sd_many_plan (host-only): (chunk_base [R] int64, total_chunks) of the packed layout of sd_diarize_many* for recordings of these lengths"""
    n = np.ascontiguousarray(lengths, np.int64)
    base = np.zeros(len(n), np.int64)
    total = C.c_int64(0)
    rc = lib().sd_many_plan(_ptr(n) if len(n) else None, len(n), _ptr(base) if len(n) else None, C.addressof(total))
    if rc:
        raise SdError(rc, "sd_many_plan: bad argument")
    return base, total.value


def sample_rows(rows, max_num, seed=0):
    """sd_sample_rows (host-only): the rows of an ascending list that a clustering call under max_num_embeddings = max_num and clustering_seed = seed
    keeps as its train rows (all of them under -1 or when there are no more than max_num), ascending, int32"""
    r = np.ascontiguousarray(rows, np.int32).reshape(-1)
    out = np.zeros(max(len(r), 1), np.int32)
    m = lib().sd_sample_rows(_ptr(r) if len(r) else None, len(r), int(max_num), int(seed), _ptr(out))
    if m < 0:
        raise SdError(-m, "sd_sample_rows: bad argument (rows ascending, distinct and >= 0; max_num -1 or >= 1)")
    return out[:m].copy()


def convert_onnx(onnx_path, kind, out_path):
    """kind: 'segmentation' | 'embedding'.  Host-only (no GPU needed)."""
    rc = lib().sd_convert_onnx(onnx_path.encode(), 0 if kind.startswith('seg') else 1, out_path.encode())
    if rc:
        raise SdError(rc, lib().sd_convert_error().decode())


def format_turn(t):
    tt = Turn(t[0], t[1], t[2], 0)
    buf = C.create_string_buffer(128)
    lib().sd_format_turn(C.byref(tt), buf, 128)
    return buf.value.decode()


def read_wav(path):
    p = C.POINTER(C.c_int16)()
    n, sr, ch = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    rc = lib().sd_read_wav(path.encode(), C.byref(p), C.byref(n), C.byref(sr), C.byref(ch))
    if rc:
        raise SdError(rc, "cannot read wav " + path)
    total = n.value * max(ch.value, 1)
    arr = np.ctypeslib.as_array(p, shape=(total,)).copy()
    lib().sd_free_pcm(p)
    return arr[:n.value], sr.value, ch.value


def read_wav_f32(path):
    """8/16/32-bit PCM -> float32 samples / 32768 (reference scaling), sample_rate, channels, bits"""
    p = C.POINTER(C.c_float)()
    n, sr, ch, bits = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = lib().sd_read_wav_f32(path.encode(), C.byref(p), C.byref(n), C.byref(sr), C.byref(ch), C.byref(bits))
    if rc:
        raise SdError(rc, "cannot read wav " + path)
    total = n.value * max(ch.value, 1)
    arr = np.ctypeslib.as_array(p, shape=(total,)).copy()
    lib().sd_free_wav(p)
    return arr[:n.value], sr.value, ch.value, bits.value


def g711_decode(encoding, codes):
    """sd_g711_decode (host-only): uint8 codes of ENC_MULAW / ENC_ALAW -> the int16 values of ITU-T G.711's tables"""
    codes = np.ascontiguousarray(codes, np.uint8).reshape(-1)
    out = np.zeros(len(codes), np.int16)
    rc = lib().sd_g711_decode(int(encoding), _ptr(codes) if len(codes) else None, len(codes), _ptr(out) if len(codes) else None)
    if rc != 0:
        raise SdError(rc, "sd_g711_decode: bad argument")
    return out


def audio_len16(audio):
    """sd_audio_len16 (host-only): the 16 kHz samples an Audio defines, -1 for a bad descriptor"""
    d = audio.desc()
    return int(lib().sd_audio_len16(C.byref(d)))


def read_wav_audio(path):
    """sd_read_wav_audio (host-only): a wav of 16-bit PCM, mu-law or A-law as an Audio holding the file's own bytes (channel = 0)"""
    d, p = AudioDesc(), C.c_void_p()
    rc = lib().sd_read_wav_audio(str(path).encode(), C.byref(d), C.byref(p))
    if rc != 0:
        raise SdError(rc, "cannot read wav as audio " + str(path))
    dt = _ENC_DTYPES[d.encoding]
    count = d.n * d.channels
    data = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(count * np.dtype(dt).itemsize, 1),))[:count * np.dtype(dt).itemsize].copy().view(dt)
    lib().sd_free_pcm(C.cast(p, C.POINTER(C.c_int16)))
    return Audio(data, d.sample_rate, d.encoding, d.channels, d.channel, n=d.n)


def _turn_array(turns):
    arr = (Turn * max(len(turns), 1))()
    for i, t in enumerate(turns):
        arr[i] = Turn(t[0], t[1], t[2], 0)
    return arr


def write_rttm(path, uri, turns, conf=None):
    arr = _turn_array(turns)
    if conf is None:
        rc = lib().sd_write_rttm(path.encode(), uri.encode(), arr, len(turns))
    else:
        cc = (C.c_double * max(len(turns), 1))(*[float(x) for x in conf])
        rc = lib().sd_write_rttm_ex(path.encode(), uri.encode(), arr, len(turns), cc)
    if rc:
        raise SdError(rc, "cannot write " + path)


DER_COMPONENTS = ("total", "missed", "false_alarm", "confusion", "correct")


def der(ref, hyp, uem=None, collar=0.0, skip_overlap=False):
    """sd_der: the diarization error rate of hypothesis turns against reference turns ([(start, end, label)], labels >= 0) by the rule of
    pyannote.metrics' DiarizationErrorRate (include/sdhip.h).  uem: [(start, end)] spans that are scored, None = everything.  Returns a dict: der,
    total, missed, false_alarm, confusion, correct (seconds) and map = {hypothesis label: reference label} of the optimal pairing.  Host-only."""
    r, h = _turn_array(ref), _turn_array(hyp)
    u, nu = _span_array(uem)
    cap = max([int(t[2]) for t in hyp if int(t[2]) >= 0] + [-1]) + 1
    m = (C.c_int32 * max(cap, 1))()
    out, nm = DerResult(), C.c_int64(0)
    rc = lib().sd_der(r, len(ref), h, len(hyp), u, nu, float(collar), 1 if skip_overlap else 0, C.byref(out), m, cap, C.byref(nm))
    if rc:
        raise SdError(rc, lib().sd_score_error().decode())
    res = {k: getattr(out, k) for k in ("der",) + DER_COMPONENTS}
    res["map"] = {k: int(m[k]) for k in range(min(cap, nm.value)) if m[k] >= 0}
    return res


def read_rttm(path, uri=None):
    """sd_read_rttm: the SPEAKER lines of an RTTM file (of one uri, or of all) -> (turns [(start, end, label)], names): label k is names[k], numbered in
    order of first appearance.  Host-only; a malformed line raises with its line number."""
    p, n, names, K = C.POINTER(Turn)(), C.c_int64(0), C.POINTER(C.c_char_p)(), C.c_int64(0)
    rc = lib().sd_read_rttm(str(path).encode(), None if uri is None else str(uri).encode(), C.byref(p), C.byref(n), C.byref(names), C.byref(K))
    if rc:
        raise SdError(rc, lib().sd_score_error().decode())
    turns = [(p[i].start, p[i].end, int(p[i].label)) for i in range(n.value)]
    out_names = [names[i].decode() for i in range(K.value)]
    lib().sd_free_turns(p)
    lib().sd_free_rttm_names(names, K)
    return turns, out_names


def read_voiceprints(path):
    """sd_read_voiceprints: a voiceprint file -> (names, emb [M][192] float64).  Host-only; a malformed line raises with its line number."""
    names, emb, M = C.POINTER(C.c_char_p)(), C.POINTER(C.c_double)(), C.c_int64(0)
    rc = lib().sd_read_voiceprints(str(path).encode(), C.byref(names), C.byref(emb), C.byref(M))
    if rc:
        raise SdError(rc, lib().sd_voiceprints_error().decode())
    out_names = [names[i].decode() for i in range(M.value)]
    out = np.ctypeslib.as_array(emb, shape=(M.value, EMB_DIM)).copy() if M.value else np.zeros((0, EMB_DIM), np.float64)
    lib().sd_free_voiceprints(names, emb, M)
    return out_names, out


def write_voiceprints(path, names, emb):
    """sd_write_voiceprints: names [M] (no white space), emb [M][192] -> the text file (%.17g: reads back bit for bit).  Host-only."""
    emb = np.ascontiguousarray(emb, np.float64).reshape(-1, EMB_DIM)
    names = [str(n).encode() for n in names]
    if len(names) != len(emb):
        raise SdError(1, "write_voiceprints: %d names for %d voiceprints" % (len(names), len(emb)))
    arr = (C.c_char_p * max(len(names), 1))(*names)
    rc = lib().sd_write_voiceprints(str(path).encode(), arr, _ptr(emb), len(names))
    if rc:
        raise SdError(rc, lib().sd_voiceprints_error().decode())


def write_rttm_named(path, uri, turns, names, conf=None):
    """sd_write_rttm_named: names[k] (None = SPEAKER_kk) is the speaker field of the turns with label k"""
    arr = _turn_array(turns)
    nm = (C.c_char_p * max(len(names), 1))(*[None if n is None else str(n).encode() for n in names])
    cc = None if conf is None else (C.c_double * max(len(turns), 1))(*[float(x) for x in conf])
    rc = lib().sd_write_rttm_named(str(path).encode(), uri.encode(), arr, len(turns), cc, nm, len(names))
    if rc:
        raise SdError(rc, "cannot write " + str(path))


def _span_array(spans):
    """[(start, end[, label])] or None -> (Turn array or None, count)"""
    if spans is None:
        return None, 0
    arr = (Turn * max(len(spans), 1))()
    for i, t in enumerate(spans):
        arr[i] = Turn(float(t[0]), float(t[1]), int(t[2]) if len(t) > 2 else 0, 0)
    return arr, len(spans)


def relabel_turns(turns, mode="pyannote"):
    """'pyannote': labels that occur, sorted by their string, -> 0, 1, ... (SPEAKER_00 ...); 'first': order of first appearance"""
    arr = _turn_array(turns)
    rc = lib().sd_relabel_turns_ex(arr, len(turns), 1 if mode == "pyannote" else 0)
    if rc:
        raise SdError(rc, "sd_relabel_turns_ex: bad argument")
    return [(arr[i].start, arr[i].end, int(arr[i].label)) for i in range(len(turns))]


def relabel_turns_map(turns, ids):
    """sd_relabel_turns_map: the label k of every turn becomes ids[k] (Diarizer.last_roster_ids, Roster.update*); times and order stay.  A label outside
    [0, len(ids)) raises SdError and nothing is renamed"""
    arr = _turn_array(turns)
    ids = np.ascontiguousarray(ids, np.int32)
    rc = lib().sd_relabel_turns_map(arr, len(turns), _ptr(ids) if len(ids) else None, len(ids))
    if rc:
        raise SdError(rc, "sd_relabel_turns_map: a label outside the map")
    return [(arr[i].start, arr[i].end, int(arr[i].label)) for i in range(len(turns))]


class Roster:
    """sd_roster_*: persistent speaker ids.  update() is the rule of include/sdhip.h on centroids and counts (and, optionally, row labels); update_last()
    names the label columns of a Diarizer's last job; Stream.set_roster makes a stream's turns carry roster ids.  Host only: no GPU, no Diarizer needed."""

    def __init__(self, d=EMB_DIM):
        h = C.c_void_p(None)
        rc = lib().sd_roster_open(int(d), C.byref(h))
        if rc:
            raise SdError(rc, "sd_roster_open: bad argument")
        self._r = h
        self.d = int(d)

    def _handle(self):
        if not self._r:
            raise SdError(1, "the roster is closed")
        return self._r

    def close(self):
        """sd_roster_close: raises SdError(1) while a stream still holds the roster"""
        if self._r:
            rc = lib().sd_roster_close(self._r)
            if rc:
                raise SdError(rc, "sd_roster_close: a stream is still attached")
            self._r = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, centroids, counts):
        """sd_roster_load: entries 0 .. P-1 into an empty roster"""
        cen = np.ascontiguousarray(centroids, np.float64).reshape(-1, self.d)
        cnt = np.ascontiguousarray(counts, np.int64)
        if len(cnt) != len(cen):
            raise SdError(1, "one count per centroid")
        rc = lib().sd_roster_load(self._handle(), _ptr(cen) if len(cen) else None, _ptr(cnt) if len(cen) else None, len(cen))
        if rc:
            raise SdError(rc, "sd_roster_load: bad argument, or the roster is not empty")

    def info(self):
        """(entries P, updates so far, dimensions)"""
        P, U, d = C.c_int64(0), C.c_int64(0), C.c_int(0)
        lib().sd_roster_info(self._handle(), C.byref(P), C.byref(U), C.byref(d))
        return int(P.value), int(U.value), int(d.value)

    def speakers(self):
        """sd_roster_speakers: (centroids [P][d] float64, counts [P] int64, seen [P] int64 = the index of the last update that gave the entry out, -1: never)"""
        P = self.info()[0]
        cen, cnt, seen = np.zeros((P, self.d), np.float64), np.zeros(P, np.int64), np.zeros(P, np.int64)
        if P:
            lib().sd_roster_speakers(self._handle(), _ptr(cen), _ptr(cnt), _ptr(seen), P, None)
        return cen, cnt, seen

    def update(self, centroids, counts, rows=None, prev=None, shift=0, threshold=None):
        """sd_roster_update: ids [K] int32 of the K label columns; rows / prev = the hard labels of this job's rows and the ids the previous update gave
        the rows of its table (row i now = row i + shift then); threshold None = the constant t * t / 2"""
        cen = np.ascontiguousarray(centroids, np.float64).reshape(-1, self.d)
        cnt = np.ascontiguousarray(counts, np.int64)
        K = len(cen)
        if len(cnt) != K:
            raise SdError(1, "one count per centroid")
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32).reshape(-1)
        prev = None if prev is None else np.ascontiguousarray(prev, np.int32).reshape(-1)
        ids = np.zeros(K, np.int32)
        keep = np.zeros(1, np.int32)                  # (an empty array has no address worth passing: absent and empty are different things here)
        rc = lib().sd_roster_update(self._handle(), _ptr(cen) if K else None, _ptr(cnt) if K else None, K,
                                    None if rows is None else _ptr(rows if len(rows) else keep), 0 if rows is None else len(rows),
                                    None if prev is None else _ptr(prev if len(prev) else keep), 0 if prev is None else len(prev), int(shift),
                                    float("nan") if threshold is None else float(threshold), _ptr(ids) if K else None)
        if rc:
            raise SdError(rc, "sd_roster_update: %s" % {1: "bad argument", 5: "zero-norm centroid", 7: "out of memory"}.get(rc, "failed"))
        return ids

    def update_last(self, diarizer):
        """sd_roster_update_last: ids [K] int32 of the label columns of the diarizer's last job (after many_select(r): of recording r), by centroid alone"""
        K = C.c_int64(0)
        diarizer._chk(lib().sd_last_speakers(diarizer._h, None, 0, C.byref(K), None))
        ids = np.zeros(max(K.value, 1), np.int32)
        diarizer._chk(lib().sd_roster_update_last(self._handle(), diarizer._h, _ptr(ids), K.value, C.byref(K)))
        return ids[:K.value].copy()


def comm_unique_id():
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().sd_comm_unique_id(buf)
    if rc:
        raise SdError(rc, "sd_comm_unique_id failed (RCCL needs a GPU)")
    return buf.raw


class Stream:
    """sd_stream_*: a recording that is still growing.  push* appends samples (and infers the blocks of 32 chunks that became final),
    turns() == Diarizer.diarize of everything pushed so far.  Made by Diarizer.stream(); also a context manager."""

    def __init__(self, diarizer):
        self._d = diarizer
        h = C.c_void_p(None)
        diarizer._chk(lib().sd_stream_open(diarizer._h, C.byref(h)))
        self._s = h

    def close(self):
        if self._s and self._d._h:              # a closed Diarizer has closed its streams (sd_destroy)
            lib().sd_stream_close(self._s)
        self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._s or not self._d._h:
            raise SdError(1, "the stream is closed")
        return self._s

    def push(self, pcm):
        pcm = np.ascontiguousarray(pcm, np.int16)
        self._d._chk(lib().sd_stream_push(self._handle(), _ptr(pcm), len(pcm)))

    def push_f32(self, wav):
        wav = np.ascontiguousarray(wav, np.float32)
        self._d._chk(lib().sd_stream_push_f32(self._handle(), _ptr(wav), len(wav)))

    def push_dev(self, d_pcm_ptr, n_samples):
        self._d._chk(lib().sd_stream_push_dev(self._handle(), C.c_void_p(d_pcm_ptr or None), n_samples))

    def turns(self):
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._d._chk(lib().sd_stream_turns(self._handle(), C.byref(p), C.byref(n)))
        return self._d._clustered(p, n)

    def info(self):
        """(samples pushed, chunks sealed, chunks in all)"""
        n, sealed, total = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._d._chk(lib().sd_stream_info(self._handle(), C.byref(n), C.byref(sealed), C.byref(total)))
        return int(n.value), int(sealed.value), int(total.value)

    def forget(self, keep_blocks):
        """sd_stream_forget: all but the last keep_blocks sealed blocks of 32 chunks go; afterwards the stream is a new one fed the kept samples"""
        self._d._chk(lib().sd_stream_forget(self._handle(), int(keep_blocks)))

    def set_window(self, keep_blocks):
        """sd_stream_set_window: every push that seals a block forgets down to keep_blocks blocks (-1: no window)"""
        self._d._chk(lib().sd_stream_set_window(self._handle(), int(keep_blocks)))

    def set_roster(self, roster):
        """sd_stream_set_roster: from now on turns() carries the roster's ids (Diarizer.last_roster_ids gives the map); None detaches"""
        self._d._chk(lib().sd_stream_set_roster(self._handle(), None if roster is None else roster._handle()))
        self._roster = roster                  # (keeps the object alive as long as the stream names it)

    def origin(self):
        """sd_stream_origin: samples forgotten so far = the sample of everything pushed at which the stream's times start"""
        o = C.c_int64(0)
        self._d._chk(lib().sd_stream_origin(self._handle(), C.byref(o)))
        return int(o.value)

    def set_input_rate(self, sr):
        """sd_stream_set_input_rate: from now on every push hands over samples at sr Hz (before the first sample only; 16000 = no resampler)"""
        self._d._chk(lib().sd_stream_set_input_rate(self._handle(), int(sr)))

    def end_input(self):
        """sd_stream_end_input: the outputs behind the last final one, with silence behind the last input as Diarizer.resample has it; no push afterwards"""
        self._d._chk(lib().sd_stream_end_input(self._handle()))

    def input_info(self):
        """sd_stream_input_info: (input rate, inputs pushed, outputs final so far, input closed)"""
        sr, closed = C.c_int32(0), C.c_int32(0)
        n_in, n_final = C.c_int64(0), C.c_int64(0)
        self._d._chk(lib().sd_stream_input_info(self._handle(), C.byref(sr), C.byref(n_in), C.byref(n_final), C.byref(closed)))
        return int(sr.value), int(n_in.value), int(n_final.value), int(closed.value)

    def set_input_format(self, encoding, channels=1, channel=0):
        """sd_stream_set_input_format: from now on the stream takes interleaved frames of `channels` elements in `encoding` (ENC_*) through push_audio*,
        one channel of them or, with channel -1, their mean (before the first sample only, in either order with set_input_rate)"""
        self._d._chk(lib().sd_stream_set_input_format(self._handle(), int(encoding), int(channels), int(channel)))

    def input_format(self):
        """sd_stream_input_format: (encoding, channels, channel, whether a format was set)"""
        v = [C.c_int32(0) for _ in range(4)]
        self._d._chk(lib().sd_stream_input_format(self._handle(), *[C.byref(q) for q in v]))
        return tuple(int(q.value) for q in v)

    def _frames_of(self, data):
        """(the array, flat and contiguous; the frames it holds).  Nothing is converted: on a stream with a format an array of another dtype than the
        format's (int16, float32, uint8 for G.711) or one that ends in a partial frame is refused here with SD_ERR_ARG, and an array that is already
        contiguous is not copied, so the same array gives the same pointer.  A stream without a format hands its elements on as they are, for the
        library to refuse."""
        enc, channels, _, is_set = self.input_format()
        data = np.asarray(data)
        if is_set and data.dtype != _ENC_DTYPES[enc]:
            raise SdError(1, "push_audio: the stream's format takes %s elements, the array holds %s" % (np.dtype(_ENC_DTYPES[enc]).name, data.dtype.name))
        data = np.ascontiguousarray(data).reshape(-1)
        if is_set and len(data) % channels:
            raise SdError(1, "push_audio: %d elements are no whole number of frames of %d channels" % (len(data), channels))
        return data, len(data) // channels if is_set else len(data)

    def push_audio(self, data):
        """sd_stream_push_audio: whole interleaved frames in the stream's format, in an array of the format's dtype (int16, float32, or one G.711
        code per uint8); another dtype or a partial frame is refused, nothing is converted"""
        data, frames = self._frames_of(data)
        self._d._chk(lib().sd_stream_push_audio(self._handle(), _ptr(data) if data.size else None, frames))

    def push_audio_dev(self, d_ptr, frames):
        """sd_stream_push_audio_dev: a device pointer to `frames` interleaved frames in the stream's format"""
        self._d._chk(lib().sd_stream_push_audio_dev(self._handle(), C.c_void_p(d_ptr or None), int(frames)))

    def _tail(self):
        """sd_test_stream_tail: (the f32 samples the stream holds on the device, from sample sealed * 8000 on; the index of the first of them)"""
        n, first = C.c_int64(0), C.c_int64(0)
        self._d._chk(lib().sd_test_stream_tail(self._handle(), None, 0, C.byref(n), C.byref(first)))
        out = np.zeros(max(n.value, 1), np.float32)
        self._d._chk(lib().sd_test_stream_tail(self._handle(), _ptr(out), len(out), C.byref(n), C.byref(first)))
        return out[:n.value], int(first.value)

    def read(self, lo, hi, seg=True, emb=True):
        """cached rows of chunks [lo, hi): (scores [hi-lo][293][3] or None, embeddings [(hi-lo)*3][192] or None)"""
        rows = max(int(hi) - int(lo), 0)
        s = np.zeros((rows, FRAMES, SPEAKERS), np.float32) if seg else None
        e = np.zeros((rows * SPEAKERS, EMB_DIM), np.float32) if emb else None
        self._d._chk(lib().sd_stream_read(self._handle(), int(lo), int(hi), _ptr(s) if seg else None, _ptr(e) if emb else None))
        return s, e


class Cut:
    """sd_cut_*: one dendrogram, many cuts.  Opening runs everything of a finalize that does not depend on clustering_threshold, min_cluster_size and
    num_clusters -- the linkage above all -- once; turns_many evaluates any number of cuts on it, each equal to Diarizer.finalize_dev under those options.
    Made by Diarizer.cut_open*; also a context manager."""

    def __init__(self, diarizer, handle):
        self._d = diarizer
        self._k = handle

    def close(self):
        if self._k and self._d._h:              # a closed Diarizer has closed its cuts (sd_destroy)
            lib().sd_cut_close(self._k)
        self._k = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._k or not self._d._h:
            raise SdError(1, "the cut is closed")
        return self._k

    @staticmethod
    def _spec(s):
        """(threshold, min_cluster_size, num_clusters), a dict of them or None; None / missing = the context's current option"""
        if s is None:
            s = {}
        if isinstance(s, dict):
            s = (s.get("threshold"), s.get("min_cluster_size"), s.get("num_clusters"))
        s = tuple(s) + (None,) * (3 - len(s))
        return CutSpec(float("nan") if s[0] is None else float(s[0]), 0 if s[1] is None else int(s[1]), 0 if s[2] is None else int(s[2]))

    def turns_many(self, specs, with_k=False):
        """sd_cut_turns_many: the turns of every spec (see _spec) in one call; with_k: (turns, K) pairs"""
        T = len(specs)
        arr = (CutSpec * max(T, 1))(*[self._spec(s) for s in specs])
        tp, nt, K = (C.POINTER(Turn) * max(T, 1))(), (C.c_int64 * max(T, 1))(), (C.c_int32 * max(T, 1))()
        self._d._chk(lib().sd_cut_turns_many(self._handle(), arr, T, tp, nt, K))
        self._d._last_d = EMB_DIM
        out = []
        for t in range(T):
            turns = [(tp[t][i].start, tp[t][i].end, int(tp[t][i].label)) for i in range(nt[t])]
            lib().sd_free_turns(tp[t])
            out.append((turns, int(K[t])) if with_k else turns)
        return out

    def turns(self, threshold=None, min_cluster_size=None, num_clusters=None):
        """sd_cut_turns: one cut"""
        p, n = C.POINTER(Turn)(), C.c_int64(0)
        spec = self._spec((threshold, min_cluster_size, num_clusters))
        self._d._chk(lib().sd_cut_turns(self._handle(), C.byref(spec), C.byref(p), C.byref(n), None))
        return self._d._clustered(p, n)

    def dendrogram(self):
        """sd_cut_dendrogram: the linkage matrix [N - 1][4] of the N train rows (N < 2: no row)"""
        N = C.c_int64(0)
        rc = lib().sd_cut_dendrogram(self._handle(), None, 0, C.byref(N))
        Z = np.zeros((max(N.value - 1, 0), 4), np.float64)
        rc = rc or lib().sd_cut_dendrogram(self._handle(), _ptr(Z) if len(Z) else None, len(Z), C.byref(N))
        if rc:
            raise SdError(rc, "sd_cut_dendrogram: bad argument")
        return Z

    def info(self):
        """(chunks, samples, train rows)"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        if lib().sd_cut_info(self._handle(), C.byref(a), C.byref(b), C.byref(c)):
            raise SdError(1, "sd_cut_info: bad argument")
        return int(a.value), int(b.value), int(c.value)


class Diarizer:
    """one libsdhip context on one GPU (not thread-safe, like the reference's OnnxModel statics)"""

    def __init__(self, seg_model=None, emb_model=None, device=0):
        L = lib()
        self._h = L.sd_create(seg_model.encode() if seg_model else None, emb_model.encode() if emb_model else None, device)
        if not self._h:
            raise SdError(-1, L.sd_create_error().decode())

    def close(self):
        if self._h:
            lib().sd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise SdError(rc, lib().sd_last_error(self._h).decode())

    def set_option(self, key, value):
        self._chk(lib().sd_set_option(self._h, key.encode(), int(value)))

    def set_option_f64(self, key, value):
        self._chk(lib().sd_set_option_f64(self._h, key.encode(), float(value)))

    def set_clustering(self, method="centroid", threshold=CLUSTERING_THRESHOLD_DEFAULT, min_cluster_size=15, max_num_embeddings=None, seed=None):
        """the three hyper-parameters of clustering/Clustering.py:251-276; the defaults are the reference's constants.  max_num_embeddings
        (Clustering.py:12, 69-76: -1 or >= 1) and seed (option "clustering_seed"): None leaves the option as it is"""
        code = _method_code(method)
        if not 0 <= code < len(LINKAGE_METHODS) or not 0.0 <= float(threshold) <= 2.0 or int(min_cluster_size) < 1:      # all three or none: the context is shared
            raise SdError(1, "set_clustering: method %r, threshold %r, min_cluster_size %r" % (method, threshold, min_cluster_size))
        if max_num_embeddings is not None and int(max_num_embeddings) != -1 and int(max_num_embeddings) < 1:
            raise SdError(1, "set_clustering: max_num_embeddings must be -1 or at least 1 (got %r)" % (max_num_embeddings,))
        if max_num_embeddings is not None:
            self.set_option("max_num_embeddings", max_num_embeddings)
        if seed is not None:
            self.set_option("clustering_seed", seed)
        self.set_option("clustering_method", code)
        self.set_option_f64("clustering_threshold", threshold)
        self.set_option("min_cluster_size", min_cluster_size)

    # ---- a2+a3
    def segment(self, wav):
        wav = np.ascontiguousarray(wav, np.float32)
        c, _ = num_chunks(len(wav))
        out = np.zeros((c, FRAMES, SPEAKERS), np.float32)
        cc = C.c_int64(0)
        self._chk(lib().sd_segment(self._h, _ptr(wav), len(wav), _ptr(out), C.byref(cc)))
        return out[:cc.value]

    # ---- a4-a6
    def postseg(self, seg):
        seg = np.ascontiguousarray(seg, np.float32)
        c = seg.shape[0]
        nb = np.zeros((c, FRAMES, SPEAKERS), np.uint8)
        masks = np.zeros((c * SPEAKERS, FRAMES), np.float32)
        cap = int(lib().sd_count_frames(c))
        count = np.zeros(max(cap, 1), np.int32)
        nc = C.c_int64(0)
        self._chk(lib().sd_postseg(self._h, _ptr(seg), c, _ptr(nb), _ptr(masks), _ptr(count), cap, C.byref(nc)))
        return nb, masks, count[:nc.value]

    def segment_chunks(self, chunks):
        """sd_segment_chunks = SegmentModel::infer as declared (sd.cpp:1352): [rows][T] separate waveforms -> ([rows][293][3], frames)"""
        chunks = np.ascontiguousarray(chunks, np.float32)
        rows, T = chunks.shape
        out = np.zeros((rows, FRAMES, SPEAKERS), np.float32)
        fr = C.c_int32(0)
        self._chk(lib().sd_segment_chunks(self._h, _ptr(chunks), rows, T, _ptr(out), C.byref(fr)))
        return out, int(fr.value)

    def embed_signals(self, signals, wav_lens):
        """sd_embed_signals = EmbeddingModel1::infer as declared (sd.cpp:1977): [B][80000] compacted signals + relative lengths -> [B][192]"""
        signals = np.ascontiguousarray(signals, np.float32)
        wav_lens = np.ascontiguousarray(wav_lens, np.float32)
        B, T = signals.shape
        assert T == 80000 and wav_lens.shape == (B,)
        out = np.zeros((B, EMB_DIM), np.float32)
        self._chk(lib().sd_embed_signals(self._h, _ptr(signals), _ptr(wav_lens), B, _ptr(out)))
        return out

    # ---- a6-a9
    def embed(self, wav, masks):
        wav = np.ascontiguousarray(wav, np.float32)
        masks = np.ascontiguousarray(masks, np.float32)
        items = masks.shape[0]
        out = np.zeros((items, EMB_DIM), np.float32)
        self._chk(lib().sd_embed(self._h, _ptr(wav), len(wav), _ptr(masks), items, _ptr(out)))
        return out

    def frontend(self, wav, masks):
        wav = np.ascontiguousarray(wav, np.float32)
        masks = np.ascontiguousarray(masks, np.float32)
        items = masks.shape[0]
        feats = np.zeros((items, T_FRAMES, N_MELS), np.float32)
        lens = np.zeros(items, np.float32)
        self._chk(lib().sd_frontend(self._h, _ptr(wav), len(wav), _ptr(masks), items, _ptr(feats), _ptr(lens)))
        return feats, lens

    def ecapa(self, feats, lens):
        feats = np.ascontiguousarray(feats, np.float32)
        lens = np.ascontiguousarray(lens, np.float32)
        items = feats.shape[0]
        out = np.zeros((items, EMB_DIM), np.float32)
        self._chk(lib().sd_ecapa(self._h, _ptr(feats), _ptr(lens), items, _ptr(out)))
        return out

    # ---- a12-a14
    def linkage(self, X):
        X = np.ascontiguousarray(X, np.float64)
        N, d = X.shape
        Z = np.zeros((max(N - 1, 0), 4), np.float64)
        self._chk(lib().sd_linkage(self._h, _ptr(X), N, d, _ptr(Z)))
        return Z

    def cluster(self, X, cutoff):
        X = np.ascontiguousarray(X, np.float64)
        N, d = X.shape
        T = np.zeros(N, np.int32)
        self._chk(lib().sd_cluster(self._h, _ptr(X), N, d, float(cutoff), _ptr(T)))
        return T

    def linkage_ex(self, X, method, metric=METRIC_EUCLIDEAN):
        """sd_linkage_ex: method = a name of LINKAGE_METHODS or its code; metric = METRIC_EUCLIDEAN / METRIC_COSINE"""
        X = np.ascontiguousarray(X, np.float64)
        N, d = X.shape
        Z = np.zeros((max(N - 1, 0), 4), np.float64)
        self._chk(lib().sd_linkage_ex(self._h, _ptr(X), N, d, _method_code(method), int(metric), _ptr(Z)))
        return Z

    def linkage_many(self, Xs, method, metric=METRIC_EUCLIDEAN):
        """sd_linkage_many: Xs = a list of [N_j][d] arrays (N_j >= 0, one d) -> (list of Z [max(N_j - 1, 0)][4], status [J] int32).  The Z of a job whose
        status is not 0 (a zero-norm row under the cosine metric) is all NaN"""
        Xs = [np.ascontiguousarray(X, np.float64).reshape(len(X), -1) for X in Xs]
        d = max([X.shape[1] for X in Xs if X.shape[0]] or [1])
        if any(X.shape[0] and X.shape[1] != d for X in Xs):
            raise ValueError("linkage_many: every job needs rows of the same length")
        N = np.array([X.shape[0] for X in Xs], np.int64)
        allX = np.ascontiguousarray(np.concatenate([X.reshape(-1, d) for X in Xs]) if len(Xs) else np.zeros((0, d)))
        nz = np.maximum(N - 1, 0)
        Z = np.full((int(nz.sum()) + 1, 4), np.nan)
        status = np.zeros(len(Xs), np.int32)
        self._chk(lib().sd_linkage_many(self._h, _ptr(allX), _ptr(N), len(Xs), d, _method_code(method), int(metric), _ptr(Z), _ptr(status)))
        off = np.concatenate([[0], np.cumsum(nz)])
        return [Z[off[j]:off[j + 1]].copy() for j in range(len(Xs))], status

    def cluster_ex(self, X, method, metric, cutoff):
        X = np.ascontiguousarray(X, np.float64)
        N, d = X.shape
        T = np.zeros(N, np.int32)
        self._chk(lib().sd_cluster_ex(self._h, _ptr(X), N, d, _method_code(method), int(metric), float(cutoff), _ptr(T)))
        return T

    def clustering(self, emb, num_clusters=-1, min_clusters=-1, max_clusters=-1):
        emb = np.ascontiguousarray(emb, np.float64)
        c, S, d = emb.shape
        assert S == SPEAKERS
        hard = np.zeros((c, S), np.int32)
        K = C.c_int32(0)
        self._chk(lib().sd_clustering_ex(self._h, _ptr(emb), c, d, num_clusters, min_clusters, max_clusters, _ptr(hard), C.byref(K)))
        self._last_d = d
        return hard, int(K.value)

    # ---- known speakers (sd_last_speakers, sd_span_masks, sd_voiceprint*, sd_speaker_distances, sd_match_speakers)
    def last_speakers(self):
        """sd_last_speakers: (centroids [K][d] float64, counts [K] int64) of the last call that clustered; row k = raw label k.  d = 192 unless the last
        call was clustering() on rows of another length"""
        K = C.c_int64(0)
        self._chk(lib().sd_last_speakers(self._h, None, 0, C.byref(K), None))
        d = getattr(self, "_last_d", EMB_DIM)
        cen, cnt = np.zeros((K.value, d), np.float64), np.zeros(K.value, np.int64)
        self._chk(lib().sd_last_speakers(self._h, _ptr(cen), K.value, C.byref(K), _ptr(cnt)))
        return cen, cnt

    def span_masks(self, n_samples, spans, label=-1):
        """sd_span_masks: the mask rows [chunks * 3][293] sd_voiceprint* gives the embedding stage for spans [(start, end[, label])] (None = everything)"""
        arr, ns = _span_array(spans)
        c, _ = num_chunks(int(n_samples))
        out = np.zeros((max(c, 0) * SPEAKERS, FRAMES), np.float32)
        self._chk(lib().sd_span_masks(self._h, int(n_samples), arr, ns, int(label), _ptr(out) if out.size else None))
        return out

    def _voiceprint(self, call, spans, label):
        arr, ns = _span_array(spans)
        emb, nw = np.zeros(EMB_DIM, np.float64), C.c_int64(0)
        self._chk(call(arr, ns, int(label), _ptr(emb), C.byref(nw)))
        return emb, int(nw.value)

    def voiceprint(self, pcm, spans=None, label=-1):
        """sd_voiceprint: (embedding [192] float64, windows averaged) of the samples of `pcm` inside the spans with this label (label < 0: all)"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        return self._voiceprint(lambda *a: lib().sd_voiceprint(self._h, _ptr(pcm), len(pcm), *a), spans, label)

    def voiceprint_dev(self, d_pcm_ptr, n_samples, spans=None, label=-1):
        return self._voiceprint(lambda *a: lib().sd_voiceprint_dev(self._h, C.c_void_p(d_pcm_ptr or None), n_samples, *a), spans, label)

    def voiceprint_f32(self, wav, spans=None, label=-1):
        wav = np.ascontiguousarray(wav, np.float32)
        return self._voiceprint(lambda *a: lib().sd_voiceprint_f32(self._h, _ptr(wav), len(wav), *a), spans, label)

    def voiceprint_wav(self, path, spans=None, label=-1, resample=False, downmix=False, assume_16k=False):
        flags = (1 if resample else 0) | (2 if downmix else 0) | (4 if assume_16k else 0)
        return self._voiceprint(lambda *a: lib().sd_voiceprint_wav(self._h, str(path).encode(), flags, *a), spans, label)

    def speaker_distances(self, gallery, centroids=None):
        """sd_speaker_distances: [K][M] cosine distances (sequential sums) of the centroids (None = the last job's) to the gallery rows"""
        gal = np.ascontiguousarray(gallery, np.float64)
        M, d = gal.shape
        cen = None if centroids is None else np.ascontiguousarray(centroids, np.float64)
        K = self.last_speakers()[0].shape[0] if cen is None else cen.shape[0]
        assert cen is None or cen.shape == (K, d)
        out = np.zeros((K, M), np.float64)
        self._chk(lib().sd_speaker_distances(self._h, None if cen is None else _ptr(cen), K, _ptr(gal), M, d, _ptr(out)))
        return out

    def match_speakers(self, gallery, centroids=None, threshold=None):
        """sd_match_speakers: (match [K] int32: gallery row or -1, distance [K] or NaN); threshold None = option "speaker_match_threshold" """
        gal = np.ascontiguousarray(gallery, np.float64)
        M, d = gal.shape
        cen = None if centroids is None else np.ascontiguousarray(centroids, np.float64)
        K = self.last_speakers()[0].shape[0] if cen is None else cen.shape[0]
        assert cen is None or cen.shape == (K, d)
        match, best = np.zeros(K, np.int32), np.zeros(K, np.float64)
        self._chk(lib().sd_match_speakers(self._h, None if cen is None else _ptr(cen), K, _ptr(gal), M, d,
                                          float("nan") if threshold is None else float(threshold), _ptr(match), _ptr(best)))
        return match, best

    # ---- enrolled speakers (sd_set_enrolled, sd_enrolled_info, sd_nearest_speakers, sd_last_enrolled)
    def set_enrolled(self, gallery=None):
        """sd_set_enrolled: enrol the voiceprints [M][d] for every following call of this context that clusters; None (or no row) clears the gallery"""
        if gallery is None or len(gallery) == 0:
            self._chk(lib().sd_set_enrolled(self._h, None, 0, 0))
            return
        gal = np.ascontiguousarray(gallery, np.float64)
        M, d = gal.shape
        self._chk(lib().sd_set_enrolled(self._h, _ptr(gal), M, d))

    def enrolled_info(self):
        """sd_enrolled_info: (rows, dimensions) of the enrolled gallery, (0, 0) when there is none"""
        M, d = C.c_int64(0), C.c_int(0)
        self._chk(lib().sd_enrolled_info(self._h, C.byref(M), C.byref(d)))
        return int(M.value), int(d.value)

    def nearest_speakers(self, X, gallery=None):
        """sd_nearest_speakers: (best [N] int32, dist [N] float64) = the nearest gallery row (first minimum) of every row of X [N][d] and its cosine
        distance; gallery None = the enrolled one"""
        X = np.ascontiguousarray(X, np.float64)
        N, d = X.shape
        if gallery is None:
            gal, (M, _) = None, self.enrolled_info()
        else:
            gal = np.ascontiguousarray(gallery, np.float64)
            M = gal.shape[0]
            assert gal.ndim == 2 and gal.shape[1] == d
        best, dist = np.zeros(N, np.int32), np.zeros(N, np.float64)
        self._chk(lib().sd_nearest_speakers(self._h, _ptr(X), N, None if gal is None else _ptr(gal), M, d, _ptr(best), _ptr(dist)))
        return best, dist

    def last_enrolled(self):
        """sd_last_enrolled: [K] int32, the gallery row of every label of the last call that clustered, -1 for a speaker nobody enrolled"""
        K = C.c_int64(0)
        self._chk(lib().sd_last_enrolled(self._h, None, 0, C.byref(K)))
        rows = np.full(K.value, -1, np.int32)
        self._chk(lib().sd_last_enrolled(self._h, _ptr(rows) if K.value else None, K.value, C.byref(K)))
        return rows

    def last_roster_ids(self):
        """sd_last_roster_ids: [K] int32, the roster id of every raw label of the last job (they name last_speakers' rows); empty when no roster took part"""
        K = C.c_int64(0)
        self._chk(lib().sd_last_roster_ids(self._h, None, 0, C.byref(K)))
        ids = np.zeros(K.value, np.int32)
        self._chk(lib().sd_last_roster_ids(self._h, _ptr(ids) if K.value else None, K.value, C.byref(K)))
        return ids

    # ---- a15-a17
    def reconstruct(self, seg, binarized, hard, count, n_samples):
        seg = np.ascontiguousarray(seg, np.float32)
        binarized = np.ascontiguousarray(binarized, np.uint8)
        hard = np.ascontiguousarray(hard, np.int32)
        count = np.ascontiguousarray(count, np.int32)
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_reconstruct(self._h, _ptr(seg), _ptr(binarized), _ptr(hard), _ptr(count), len(count),
                                       seg.shape[0], n_samples, C.byref(p), C.byref(n)))
        return self._turns(p, n)

    def _turns(self, p, n):
        out = [(p[i].start, p[i].end, int(p[i].label)) for i in range(n.value)]
        if p:
            lib().sd_free_turns(p)
        return out

    def _clustered(self, p, n):
        """turns of a call that clustered 192-dimensional embeddings (last_speakers reads the row length)"""
        self._last_d = EMB_DIM
        return self._turns(p, n)

    # ---- whole path
    def diarize(self, pcm):
        pcm = np.ascontiguousarray(pcm, np.int16)
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_diarize(self._h, _ptr(pcm), len(pcm), C.byref(p), C.byref(n)))
        return self._clustered(p, n)

    def diarize_f32(self, wav):
        wav = np.ascontiguousarray(wav, np.float32)
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_diarize_f32(self._h, _ptr(wav), len(wav), C.byref(p), C.byref(n)))
        return self._clustered(p, n)

    def set_dump_dir(self, path, level=1):
        """sd_set_dump_dir: the reference's WRITE_DATA items as <path>/cpp_<item>.txt from the next whole-path call on (None = off)"""
        self._chk(lib().sd_set_dump_dir(self._h, str(path).encode() if path else None, level if path else 0))

    def diarize_wav(self, path, resample=False, downmix=False, assume_16k=False):
        """sd_diarize_wav: reader + sample-rate / channel handling + the whole path (SD_WAV_RESAMPLE = 1, SD_WAV_DOWNMIX = 2, SD_WAV_ASSUME_16K = 4)"""
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_diarize_wav(self._h, str(path).encode(), (1 if resample else 0) | (2 if downmix else 0) | (4 if assume_16k else 0), C.byref(p), C.byref(n)))
        return self._clustered(p, n)

    def resample(self, wav, in_sr, out_sr=16000):
        wav = np.ascontiguousarray(wav, np.float32)
        no = C.c_int64(0)
        self._chk(lib().sd_resample(self._h, _ptr(wav), len(wav), in_sr, out_sr, None, 0, C.byref(no)))
        out = np.zeros(max(no.value, 1), np.float32)
        self._chk(lib().sd_resample(self._h, _ptr(wav), len(wav), in_sr, out_sr, _ptr(out), len(out), C.byref(no)))
        return out[:no.value]

    def diarize_dev(self, d_pcm_ptr, n_samples):
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_diarize_dev(self._h, C.c_void_p(d_pcm_ptr), n_samples, C.byref(p), C.byref(n)))
        return self._clustered(p, n)

    def _many(self, fn, ptrs, lengths):
        """one sd_diarize_many* call -> per recording the turns, or the error code (SD_ERR_SHORT = 4, SD_ERR_NUMERIC = 5) it ended with"""
        R = len(ptrs)
        rows = (C.c_void_p * max(R, 1))(*ptrs)
        n = (C.c_int64 * max(R, 1))(*[int(v) for v in lengths])
        turns = (C.POINTER(Turn) * max(R, 1))()
        nt = (C.c_int64 * max(R, 1))()
        status = (C.c_int32 * max(R, 1))()
        self._chk(fn(self._h, rows, n, R, turns, nt, status))
        self._last_d = EMB_DIM
        out = []
        for r in range(R):
            t = self._turns(turns[r], C.c_int64(nt[r]))
            out.append(t if status[r] == 0 else int(status[r]))
        return out

    def diarize_many(self, recordings):
        """sd_diarize_many: int16 recordings -> list of (turns | error code), each what diarize() gives for that recording alone"""
        recs = [np.ascontiguousarray(p, np.int16) for p in recordings]
        return self._many(lib().sd_diarize_many, [p.ctypes.data for p in recs], [len(p) for p in recs])

    def diarize_many_f32(self, recordings):
        recs = [np.ascontiguousarray(p, np.float32) for p in recordings]
        return self._many(lib().sd_diarize_many_f32, [p.ctypes.data for p in recs], [len(p) for p in recs])

    def diarize_many_dev(self, d_pcm_ptrs, lengths):
        """sd_diarize_many_dev: device pointers of int16 recordings and their lengths"""
        return self._many(lib().sd_diarize_many_dev, [int(p) for p in d_pcm_ptrs], lengths)

    def _many_audio(self, fn, recordings):
        R = len(recordings)
        arr = (AudioDesc * max(R, 1))(*[a.desc() for a in recordings])
        turns = (C.POINTER(Turn) * max(R, 1))()
        nt = (C.c_int64 * max(R, 1))()
        status = (C.c_int32 * max(R, 1))()
        self._chk(fn(self._h, arr, R, turns, nt, status))
        self._last_d = EMB_DIM
        out = []
        for r in range(R):
            t = self._turns(turns[r], C.c_int64(nt[r]))
            out.append(t if status[r] == 0 else int(status[r]))
        return out

    def diarize_many_audio(self, recordings):
        """sd_diarize_many_audio: a list of Audio in their own rate, encoding and channel layout -> list of (turns | error code), each what diarize_f32
        gives for that recording's 16 kHz mono samples alone"""
        return self._many_audio(lib().sd_diarize_many_audio, recordings)

    def diarize_many_audio_dev(self, recordings):
        """sd_diarize_many_audio_dev: the same for Audio whose data are device pointers"""
        return self._many_audio(lib().sd_diarize_many_audio_dev, recordings)

    def many_select(self, r):
        """sd_many_select: recording r of the last diarize_many* call becomes the last job of last_confidence / last_speakers / last_enrolled"""
        self._chk(lib().sd_many_select(self._h, int(r)))
        self._last_d = EMB_DIM

    def shard_infer_dev(self, d_pcm_shard_ptr, first_sample, shard_samples, n_total, chunk_lo, chunk_hi, d_seg_ptr, d_emb_ptr):
        self._chk(lib().sd_shard_infer_dev(self._h, C.c_void_p(d_pcm_shard_ptr), first_sample, shard_samples, n_total,
                                           chunk_lo, chunk_hi, C.c_void_p(d_seg_ptr), C.c_void_p(d_emb_ptr)))

    def comm_init(self, id_bytes, rank, world):
        assert len(id_bytes) == COMM_ID_BYTES
        self._chk(lib().sd_comm_init(self._h, C.c_char_p(id_bytes), rank, world))

    def comm_destroy(self):
        lib().sd_comm_destroy(self._h)

    def comm_info(self):
        r, w = C.c_int(0), C.c_int(0)
        lib().sd_comm_info(self._h, C.byref(r), C.byref(w))
        return r.value, w.value

    def diarize_sharded_dev(self, d_pcm_shard_ptr, first_sample, shard_samples, n_total):
        """collective over the ctx's RCCL communicator; turns on rank 0, [] elsewhere"""
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_diarize_sharded_dev(self._h, C.c_void_p(d_pcm_shard_ptr or None), first_sample, shard_samples, n_total, C.byref(p), C.byref(n)))
        return self._clustered(p, n)

    def diarize_sharded(self, pcm_shard, first_sample, n_total):
        pcm_shard = np.ascontiguousarray(pcm_shard, np.int16)
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_diarize_sharded(self._h, _ptr(pcm_shard), first_sample, len(pcm_shard), n_total, C.byref(p), C.byref(n)))
        return self._clustered(p, n)

    def stream(self):
        """sd_stream_open: incremental diarization of a growing recording on this context"""
        return Stream(self)

    # ---- many streams of this context in one call
    def _push_many(self, fn, streams, ptrs, lengths):
        S = len(streams)
        if not (S == len(ptrs) == len(lengths)):
            raise SdError(1, "one pointer and one length per stream")
        hs = (C.c_void_p * max(S, 1))(*[s._handle().value for s in streams])
        rows = (C.c_void_p * max(S, 1))(*[int(p) or None for p in ptrs])
        n = (C.c_int64 * max(S, 1))(*[int(v) for v in lengths])
        rc = fn(hs, rows, n, S)
        if rc and not S:
            raise SdError(rc, "an empty list of streams")
        self._chk(rc)

    def stream_push_many(self, streams, pcms):
        """sd_stream_push_many: int16 samples for every stream of the list (an empty array: nothing for that stream), one upload and one packed inference
        of the blocks that became sealed; every stream is then what Stream.push of its own samples leaves"""
        pcms = [np.ascontiguousarray(p, np.int16) for p in pcms]
        self._push_many(lib().sd_stream_push_many, streams, [p.ctypes.data if len(p) else 0 for p in pcms], [len(p) for p in pcms])

    def stream_push_many_f32(self, streams, wavs):
        wavs = [np.ascontiguousarray(w, np.float32) for w in wavs]
        self._push_many(lib().sd_stream_push_many_f32, streams, [w.ctypes.data if len(w) else 0 for w in wavs], [len(w) for w in wavs])

    def stream_push_many_dev(self, streams, d_pcm_ptrs, lengths):
        """sd_stream_push_many_dev: device pointers of int16 samples and their lengths"""
        self._push_many(lib().sd_stream_push_many_dev, streams, d_pcm_ptrs, lengths)

    def stream_push_many_audio(self, streams, datas):
        """sd_stream_push_many_audio: interleaved frames for every stream of the list, each in its stream's format (an empty array: nothing for that
        stream), in an array of the format's dtype (another dtype or a partial frame is refused; nothing is converted or, for a contiguous array,
        copied).  The SAME array passed for two streams is the same pointer: the legs of one stereo call, uploaded once"""
        if len(streams) != len(datas):
            raise SdError(1, "one array per stream")
        rows = [s._frames_of(d) for s, d in zip(streams, datas)]      # (an array of the right type and layout is not copied: its pointer is the caller's)
        self._push_many(lib().sd_stream_push_many_audio, streams, [a.ctypes.data if a.size else 0 for a, _ in rows], [f for _, f in rows])

    def stream_push_many_audio_dev(self, streams, d_ptrs, frames):
        """sd_stream_push_many_audio_dev: device pointers of interleaved frames, each in its stream's format, and their frame counts"""
        self._push_many(lib().sd_stream_push_many_audio_dev, streams, d_ptrs, frames)

    def stream_turns_many(self, streams):
        """sd_stream_turns_many: per stream the turns Stream.turns gives, or the error code (SD_ERR_SHORT = 4, SD_ERR_NUMERIC = 5) it ended with;
        many_select(i) then makes stream i the last job"""
        S = len(streams)
        hs = (C.c_void_p * max(S, 1))(*[s._handle().value for s in streams])
        turns = (C.POINTER(Turn) * max(S, 1))()
        nt = (C.c_int64 * max(S, 1))()
        status = (C.c_int32 * max(S, 1))()
        rc = lib().sd_stream_turns_many(hs, S, turns, nt, status)
        if rc and not S:
            raise SdError(rc, "an empty list of streams")
        self._chk(rc)
        self._last_d = EMB_DIM
        out = []
        for i in range(S):
            t = self._turns(turns[i], C.c_int64(nt[i]))
            out.append(t if status[i] == 0 else int(status[i]))
        return out

    # ---- many cuts of one dendrogram
    def _cut(self, rc, h):
        self._chk(rc)
        return Cut(self, h)

    def cut_open_dev(self, d_seg_ptr, d_emb_ptr, chunks, n_samples):
        h = C.c_void_p(None)
        return self._cut(lib().sd_cut_open_dev(self._h, C.c_void_p(d_seg_ptr), C.c_void_p(d_emb_ptr), chunks, n_samples, C.byref(h)), h)

    def cut_open(self, pcm):
        pcm = np.ascontiguousarray(pcm, np.int16)
        h = C.c_void_p(None)
        return self._cut(lib().sd_cut_open(self._h, _ptr(pcm), len(pcm), C.byref(h)), h)

    def cut_open_pcm_dev(self, d_pcm_ptr, n_samples):
        h = C.c_void_p(None)
        return self._cut(lib().sd_cut_open_pcm_dev(self._h, C.c_void_p(d_pcm_ptr), n_samples, C.byref(h)), h)

    def cut_open_f32(self, wav):
        wav = np.ascontiguousarray(wav, np.float32)
        h = C.c_void_p(None)
        return self._cut(lib().sd_cut_open_f32(self._h, _ptr(wav), len(wav), C.byref(h)), h)

    def cut_open_wav(self, path, resample=False, downmix=False, assume_16k=False):
        h = C.c_void_p(None)
        return self._cut(lib().sd_cut_open_wav(self._h, str(path).encode(), (1 if resample else 0) | (2 if downmix else 0) | (4 if assume_16k else 0), C.byref(h)), h)

    def tune(self, cut, ref_turns, thresholds, min_cluster_sizes=(None,), **der_options):
        """every (threshold, min_cluster_size) of the grid -- thresholds outermost -- as one Cut.turns_many, each scored against ref_turns with der(**der_options).
        Returns (table, best): table = a list of dicts with threshold, min_cluster_size, speakers (label columns) and der's fields -- the components too, so
        that several recordings pool as the sum of errors over the sum of totals --; best = the first row with the smallest der (NaN counts as largest)."""
        grid = [(float(t), m) for t in thresholds for m in min_cluster_sizes]
        table = []
        for (t, m), (turns, K) in zip(grid, cut.turns_many([(t, m, None) for t, m in grid], with_k=True)):
            row = dict(threshold=t, min_cluster_size=m, speakers=K)
            row.update(der(ref_turns, turns, **der_options))
            table.append(row)
        best = None
        for row in table:
            if best is None or (row["der"] == row["der"] and not best["der"] <= row["der"]):
                best = row
        return table, best

    def last_confidence(self):
        n = C.c_int64(0)
        self._chk(lib().sd_last_confidence(self._h, None, 0, C.byref(n)))
        buf = (C.c_double * max(n.value, 1))()
        self._chk(lib().sd_last_confidence(self._h, buf, n.value, C.byref(n)))
        return np.array(buf[:n.value], np.float64)

    # ---- speech / overlapped-speech regions (sd_activity*)
    def set_activity(self, onset=0.5, offset=0.5, min_duration_on=0.0, min_duration_off=0.0, hamming=False):
        """pyannote's Binarize parameters of the activity timeline and the Hamming-weighted aggregation; the defaults are the library's"""
        vals = (float(onset), float(offset), float(min_duration_on), float(min_duration_off))
        if not (0.0 <= vals[0] <= 1.0 and 0.0 <= vals[1] <= 1.0 and vals[2] >= 0.0 and vals[3] >= 0.0):      # all five or none: the context is shared
            raise SdError(1, "set_activity: onset %r, offset %r, min_duration_on %r, min_duration_off %r" % vals)
        for key, v in zip(("activity_onset", "activity_offset", "activity_min_duration_on", "activity_min_duration_off"), vals):
            self.set_option_f64(key, v)
        self.set_option("activity_hamming", int(bool(hamming)))

    def activity_scores(self, seg, kind):
        """sd_activity_scores: [chunks][293][3] scores -> the aggregated speech / overlap timeline (float64, every frame)"""
        seg = np.ascontiguousarray(seg, np.float32)
        c = seg.shape[0]
        assert seg.shape == (c, FRAMES, SPEAKERS)
        nf = C.c_int64(0)
        self._chk(lib().sd_activity_scores(self._h, None, c, _activity_kind(kind), None, 0, C.byref(nf)))
        out = np.zeros(nf.value, np.float64)
        self._chk(lib().sd_activity_scores(self._h, _ptr(seg), c, _activity_kind(kind), _ptr(out), len(out), C.byref(nf)))
        return out

    def activity_regions(self, scores):
        """sd_activity_regions: a timeline -> [(start, end, 0)] by the context's activity options"""
        scores = np.ascontiguousarray(scores, np.float64).reshape(-1)
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_activity_regions(self._h, _ptr(scores), len(scores), C.byref(p), C.byref(n)))
        return self._turns(p, n)

    def activity(self, pcm, kind):
        pcm = np.ascontiguousarray(pcm, np.int16)
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_activity(self._h, _ptr(pcm), len(pcm), _activity_kind(kind), C.byref(p), C.byref(n)))
        return self._turns(p, n)

    def activity_dev(self, d_pcm_ptr, n_samples, kind):
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_activity_dev(self._h, C.c_void_p(d_pcm_ptr), n_samples, _activity_kind(kind), C.byref(p), C.byref(n)))
        return self._turns(p, n)

    def activity_f32(self, wav, kind):
        wav = np.ascontiguousarray(wav, np.float32)
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_activity_f32(self._h, _ptr(wav), len(wav), _activity_kind(kind), C.byref(p), C.byref(n)))
        return self._turns(p, n)

    def activity_wav(self, path, kind, resample=False, downmix=False, assume_16k=False):
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        flags = (1 if resample else 0) | (2 if downmix else 0) | (4 if assume_16k else 0)
        self._chk(lib().sd_activity_wav(self._h, str(path).encode(), flags, _activity_kind(kind), C.byref(p), C.byref(n)))
        return self._turns(p, n)

    def last_activity_scores(self):
        """the cropped timeline of the last whole-path activity call"""
        n = C.c_int64(0)
        self._chk(lib().sd_last_activity_scores(self._h, None, 0, C.byref(n)))
        buf = (C.c_double * max(n.value, 1))()
        self._chk(lib().sd_last_activity_scores(self._h, buf, n.value, C.byref(n)))
        return np.array(buf[:n.value], np.float64)

    def finalize_dev(self, d_seg_ptr, d_emb_ptr, chunks, n_samples):
        p = C.POINTER(Turn)()
        n = C.c_int64(0)
        self._chk(lib().sd_finalize_dev(self._h, C.c_void_p(d_seg_ptr), C.c_void_p(d_emb_ptr), chunks, n_samples,
                                        C.byref(p), C.byref(n)))
        return self._clustered(p, n)

    def set_planted(self, d_scores_ptr, d_emb_ptr, chunk_lo, chunks):
        """planted workload hook: device pointers (0 = none) for chunks [chunk_lo, chunk_lo + chunks)"""
        self._chk(lib().sd_set_planted(self._h, C.c_void_p(d_scores_ptr or None), C.c_void_p(d_emb_ptr or None), chunk_lo, chunks))

    # ---- measurement
    def stage_ms(self):
        a = (C.c_double * 4)()
        self._chk(lib().sd_stage_ms(self._h, a))
        return list(a)

    def kernel_stats(self, name):
        ms, n, fl, by = C.c_double(0), C.c_int64(0), C.c_double(0), C.c_double(0)
        self._chk(lib().sd_kernel_stats(self._h, name.encode(), C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        return {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}

    def bench_conv(self, items, Tp, T, Cin, Cout, KT=1, dil=1, has_x2=0, dbg=0, reps=5):
        ms = C.c_double(0)
        self._chk(lib().sd_bench_conv(self._h, items, Tp, T, Cin, Cout, KT, dil, has_x2, dbg, reps, C.byref(ms)))
        return ms.value

    def conv_case(self, w, x, *, n_in=None, n_out=None, tin=None, dense=None, dil=1, pad_mode=0, x2=None, bias=None, scale=None, shift=None,
                  item_bias=None, act1=0, act2=0, prec=0, y_f32=False, try_narrow=False, shared=False, x_ld=None, x_col0=0, x2_col0=0,
                  y_ld=None, y_col0=0, cin_pad=0, canary=-7776.0):
        """sd_test_conv: one conv case through the product's dispatch.  w [kt][cout][cin], x / x2 [in_rows][cin]; compact row spaces
        (n_in, n_out per item, tin) or dense=(items, tp_in, tin, tp_out, t).  Returns (the WHOLE [M + CONV_SLACK_ROWS][y_ld] output buffer
        as f32, guards included; the name of the kernel that ran).  On an error the SdError carries the kernel name ("" = nothing launched)
        as .kernel."""
        w = np.ascontiguousarray(w, np.float32)
        kt, cout, cin = w.shape
        x = np.ascontiguousarray(x, np.float32)
        k = ConvCase()
        if dense is not None:
            k.dense = 1
            k.items, k.tp_in, k.tin, k.tp_out, k.t = [int(v) for v in dense]
            M, in_rows = k.items * k.tp_out, k.items * k.tp_in
            ni = no = None
        else:
            ni, no = np.ascontiguousarray(n_in, np.int32), np.ascontiguousarray(n_out, np.int32)
            assert ni.shape == no.shape and ni.ndim == 1
            k.items, k.tin = len(ni), int(tin)
            M, in_rows = int(no.sum()), int(ni.sum())
        assert x.shape == (in_rows, cin), (x.shape, in_rows, cin)
        cpad = cin_pad or (-(-cin // 64) * 64 if prec == 1 else -(-cin // 32) * 32)
        k.cin, k.cin_pad, k.cout, k.kt, k.dil, k.pad_mode = cin, cin_pad, cout, kt, dil, pad_mode
        k.shared, k.x_col0, k.x2_col0, k.y_col0 = int(shared), x_col0, x2_col0, y_col0
        k.y_ld = int(y_ld) if y_ld is not None else y_col0 + cout
        k.x_ld = int(x_ld) if x_ld is not None else (k.y_ld if shared else x_col0 + cpad)
        k.act1, k.act2, k.prec, k.y_f32, k.try_narrow, k.canary = act1, act2, prec, int(y_f32), int(try_narrow), canary
        opt = {}
        for name, arr, shape in (("x2", x2, (in_rows, cin)), ("bias", bias, (cout,)), ("scale", scale, (cout,)), ("shift", shift, (cout,)),
                                 ("item_bias", item_bias, (k.items, cout))):
            if arr is not None:
                arr = np.ascontiguousarray(arr, np.float32)
                assert arr.shape == shape, (name, arr.shape, shape)
            opt[name] = arr
        k.has_x2 = int(x2 is not None)
        y = np.zeros((M + CONV_SLACK_ROWS, k.y_ld), np.float32)
        name = C.create_string_buffer(32)
        p = lambda a: _ptr(a) if a is not None else None
        rc = lib().sd_test_conv(self._h, C.byref(k), p(ni), p(no), _ptr(w), _ptr(x), p(opt["x2"]), p(opt["bias"]), p(opt["scale"]), p(opt["shift"]),
                                p(opt["item_bias"]), _ptr(y), name, 32)
        if rc:
            e = SdError(rc, lib().sd_last_error(self._h).decode())
            e.kernel = name.value.decode()
            raise e
        return y, name.value.decode()

    # ---- one kernel of the segmentation network alone (sdhip_test.h); each returns the WHOLE output buffer, SEG_SLACK_ROWS guard rows included
    def lstm_rec_case(self, G, whh_f, whh_b, prec=0, canary=-7776.0):
        """sd_test_lstm_rec: G [B][F][1024], whh_f / whh_b [512][128] -> H [B * F + SEG_SLACK_ROWS][256]; prec 0 = k_lstm_rec, 3 = k_lstm_rec_x3"""
        G = np.ascontiguousarray(G, np.float32)
        B, F, w = G.shape
        whh_f, whh_b = np.ascontiguousarray(whh_f, np.float32), np.ascontiguousarray(whh_b, np.float32)
        assert w == 1024 and whh_f.shape == (512, 128) and whh_b.shape == (512, 128)
        H = np.zeros((B * F + SEG_SLACK_ROWS, 256), np.float32)
        self._chk(lib().sd_test_lstm_rec(self._h, _ptr(G), _ptr(whh_f), _ptr(whh_b), B, F, int(prec), canary, _ptr(H)))
        return H

    def pool_norm_case(self, x, chunks, Lc, stage, gw, gb, cst=None, wsum=None, chunk_rows=0, canary=-7776.0):
        """sd_test_pool_norm: x [in_rows][C] (C = 80 at stage 0, 60 at stages 1 and 2) -> out [chunks * (Lc // 3) + SEG_SLACK_ROWS][96 or 64].
        cst [chunks][2] + wsum [80] + chunk_rows: the shared form of stage 0 (chunk ck starts at row ck * chunk_rows)"""
        C_, cpad = (80, 96) if stage == 0 else (60, 64)
        x = np.ascontiguousarray(x, np.float32)
        gw, gb = np.ascontiguousarray(gw, np.float32), np.ascontiguousarray(gb, np.float32)
        assert x.ndim == 2 and x.shape[1] == C_ and gw.shape == (C_,) and gb.shape == (C_,)
        if cst is not None:
            cst, wsum = np.ascontiguousarray(cst, np.float32), np.ascontiguousarray(wsum, np.float32)
            assert cst.shape == (chunks, 2) and wsum.shape == (80,)
        out = np.zeros((chunks * (Lc // 3) + SEG_SLACK_ROWS, cpad), np.float32)
        self._chk(lib().sd_test_pool_norm(self._h, _ptr(x), x.shape[0], chunks, Lc, stage, _ptr(gw), _ptr(gb), _ptr(cst) if cst is not None else None,
                                          _ptr(wsum) if cst is not None else None, int(chunk_rows), canary, _ptr(out)))
        return out

    def chunk_norm_case(self, wav, origin, first_chunk, hop, L, chunks, w, b, stats_only=False, canary=-7776.0):
        """sd_test_chunk_norm: chunk ck = wav[(first_chunk + ck) * hop - origin :][:L] -> xn [chunks * 80000 + 4 * SEG_SLACK_ROWS] (k_chunk_norm), or
        with stats_only (a, c) [chunks + SEG_SLACK_ROWS][2] (k_chunk_stats, hop = 8000)"""
        wav = np.ascontiguousarray(wav, np.float32)
        out = np.zeros((chunks + SEG_SLACK_ROWS, 2) if stats_only else (chunks * CHUNK + 4 * SEG_SLACK_ROWS,), np.float32)
        self._chk(lib().sd_test_chunk_norm(self._h, _ptr(wav), len(wav), origin, first_chunk, hop, L, chunks, w, b, int(bool(stats_only)), canary, _ptr(out)))
        return out

    def classifier_case(self, y, W, b, chunks, F, canary=-7776.0):
        """sd_test_classifier: y [chunks * F][128], W [3][128], b [3] -> seg [chunks * 293 + SEG_SLACK_ROWS][3]"""
        y, W, b = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(W, np.float32), np.ascontiguousarray(b, np.float32)
        assert y.shape == (chunks * F, 128) and W.shape == (3, 128) and b.shape == (3,)
        seg = np.zeros((chunks * FRAMES + SEG_SLACK_ROWS, 3), np.float32)
        self._chk(lib().sd_test_classifier(self._h, _ptr(y), _ptr(W), _ptr(b), chunks, F, canary, _ptr(seg)))
        return seg

    # ---- one glue kernel of the embedding network alone (sdhip_test.h); each returns the WHOLE output buffer, guard rows included
    def ecapa_stats_case(self, kind, x, nvalid, rowoff, C_, logits=None, f16=False, canary=-7776.0):
        """sd_test_ecapa_stats: kind "mean" (k_masked_mean) -> [items + GLUE_SLACK_ROWS][C]; "stats" (k_asp_stats) / "pool" (k_asp_pool, with logits)
        -> [items + GLUE_SLACK_ROWS][2 C].  x / logits [rows][ld], rows = rowoff[-1] - rowoff[0], row_base = rowoff[0]; C_ <= ld"""
        x = np.ascontiguousarray(x, np.float32)
        nv, off = np.ascontiguousarray(nvalid, np.int32), np.ascontiguousarray(rowoff, np.int32)
        items = len(nv)
        assert x.ndim == 2 and off.shape == (items + 1,) and x.shape[0] == off[-1] - off[0], (x.shape, off)
        k = {"mean": 0, "stats": 1, "pool": 2}[kind]
        if logits is not None:
            logits = np.ascontiguousarray(logits, np.float32)
            assert logits.shape == x.shape
        out = np.zeros((items + GLUE_SLACK_ROWS, C_ if k == 0 else 2 * C_), np.float32)
        self._chk(lib().sd_test_ecapa_stats(self._h, k, int(bool(f16)), _ptr(x), _ptr(logits) if logits is not None else None, _ptr(nv), _ptr(off), items,
                                            int(off[0]), int(C_), x.shape[1], canary, _ptr(out)))
        return out

    def se_apply_case(self, t2, gate, res, off, os, rs, ys, *, shared, y_ld, out_col0, res_col0=0, f16=False, canary=-7776.0):
        """sd_test_se_apply: t2 [Mo][t2_ld], gate [items][C], off [4][items + 1] prefix sums of the four row spaces; shared=False: res [rows of space rs][res_ld]
        in a buffer of its own; shared=True: res [rows of space ys][C] becomes column slice res_col0 of the output buffer.
        -> the whole [rows of space ys + GLUE_SLACK_ROWS][y_ld] buffer, the output in columns [out_col0, out_col0 + C)"""
        t2, gate, res = (np.ascontiguousarray(a, np.float32) for a in (t2, gate, res))
        off = np.ascontiguousarray(off, np.int32)
        items, C_ = gate.shape
        assert off.shape == (4, items + 1) and t2.shape[0] == off[os, -1] and res.shape[0] == off[rs, -1], (off.shape, t2.shape, res.shape)
        assert res.shape[1] == C_ if shared else res.shape[1] >= C_
        y = np.zeros((int(off[ys, -1]) + GLUE_SLACK_ROWS, y_ld), np.float32)
        self._chk(lib().sd_test_se_apply(self._h, int(bool(f16)), int(bool(shared)), _ptr(t2), t2.shape[1], _ptr(gate), _ptr(res), res.shape[1], int(res_col0),
                                         int(out_col0), int(y_ld), C_, _ptr(off), items, os, rs, ys, canary, _ptr(y)))
        return y

    def rowtab_case(self, off_out, off_in, canary=-7776):
        """sd_test_rowtab: prefix sums [items + 1] of the output and the input space (their first entries are the bases) -> [rows + ROWTAB_SLACK][2] int32"""
        oo, oi = np.ascontiguousarray(off_out, np.int32), np.ascontiguousarray(off_in, np.int32)
        assert oo.ndim == 1 and oo.shape == oi.shape
        tab = np.zeros((int(oo[-1] - oo[0]) + ROWTAB_SLACK, 2), np.int32)
        self._chk(lib().sd_test_rowtab(self._h, _ptr(oo), _ptr(oi), len(oo) - 1, canary, _ptr(tab)))
        return tab

    def scatter_emb_case(self, emb_c, cidx, canary=-7776.0):
        """sd_test_scatter_emb: emb_c [n_c][192], cidx [items] (-1 = dropped) -> [items + GLUE_SLACK_ROWS][192]"""
        emb_c, cidx = np.ascontiguousarray(emb_c, np.float32).reshape(-1, EMB_DIM), np.ascontiguousarray(cidx, np.int32)
        out = np.zeros((len(cidx) + GLUE_SLACK_ROWS, EMB_DIM), np.float32)
        self._chk(lib().sd_test_scatter_emb(self._h, _ptr(emb_c) if len(emb_c) else None, len(emb_c), _ptr(cidx), len(cidx), canary, _ptr(out)))
        return out

    def to_half_case(self, f, feats=False, canary=-7776.0):
        """sd_test_to_half: feats=True: k_feats_to_half, f [rows][96] -> fp16 [rows + GLUE_SLACK_ROWS][128]; else k_rows_to_half, f [rows][w] -> [rows + ...][w]"""
        f = np.ascontiguousarray(f, np.float32)
        rows, w = f.shape
        out = np.zeros((rows + GLUE_SLACK_ROWS, 128 if feats else w), np.uint16)
        self._chk(lib().sd_test_to_half(self._h, 0 if feats else 1, _ptr(f), rows, w, canary, _ptr(out)))
        return out.view(np.float16)

    # ---- the kernels of the embedding front end alone (sdhip_test.h); every array comes back WHOLE, its FE_SLACK entries (rows) included
    def frontend_prepare_case(self, masks, first_item=0, compact=True, icanary=-7776, fcanary=-7776.0):
        """sd_test_frontend_prepare: masks [items][293] -> dict of prefix [items * 296 + FE_SLACK], counts / wav_lens / nnorm / nvalid / flags
        [items + FE_SLACK] per item and, under compact, alist / cidx / nnorm_c / nvalid_c [items + FE_SLACK] and n_active [4]"""
        masks = np.ascontiguousarray(masks, np.float32)
        items = masks.shape[0]
        assert masks.shape == (items, 293)
        n = items + FE_SLACK
        out = {"prefix": np.zeros(items * 296 + FE_SLACK, np.int32), "wav_lens": np.zeros(n, np.float32)}
        names = ["counts", "nnorm", "nvalid", "flags"] + (["alist", "cidx", "nnorm_c", "nvalid_c"] if compact else [])
        for k in names:
            out[k] = np.zeros(n, np.int32)
        if compact:
            out["n_active"] = np.zeros(4, np.int32)
        p = lambda k: _ptr(out[k]) if k in out else None
        self._chk(lib().sd_test_frontend_prepare(self._h, _ptr(masks), items, int(first_item), int(bool(compact)), int(icanary), float(fcanary), p("prefix"),
                                                 p("counts"), p("wav_lens"), p("nnorm"), p("nvalid"), p("flags"), p("alist"), p("cidx"), p("nnorm_c"),
                                                 p("nvalid_c"), p("n_active")))
        return out

    def frontend_features_case(self, wav, n_total, origin, first_item, masks, rows_all, skip_dead_rows=True, canary=-7776.0):
        """sd_test_frontend_features: wav = samples [origin, origin + len(wav)) of a recording of n_total samples, masks [items][293], rows_all = the rows
        the caller expects the live items to store -> feats [rows_all + FE_SLACK][96], rowoff [items + 1] (n_active + 1 written), cidx [items],
        info dict (n_active, rows_all, grid, num_cu)"""
        wav, masks = np.ascontiguousarray(wav, np.float32), np.ascontiguousarray(masks, np.float32)
        items = masks.shape[0]
        assert wav.ndim == 1 and masks.shape == (items, 293)
        feats = np.zeros((int(rows_all) + FE_SLACK, 96), np.float32)
        rowoff, cidx, info = np.full(items + 1, -1, np.int32), np.zeros(items, np.int32), np.zeros(4, np.int64)
        self._chk(lib().sd_test_frontend_features(self._h, _ptr(wav), len(wav), int(n_total), int(origin), int(first_item), _ptr(masks), items,
                                                  int(bool(skip_dead_rows)), canary, _ptr(feats), feats.shape[0], _ptr(rowoff), _ptr(cidx), _ptr(info)))
        return feats, rowoff, cidx, dict(zip(("n_active", "rows_all", "grid", "num_cu"), (int(v) for v in info)))

    def frontend_signals_case(self, signals, wav_lens, rows_all, skip_dead_rows=True, icanary=-7776, canary=-7776.0):
        """sd_test_frontend_signals: signals [B][80000], wav_lens [B] -> feats [rows_all + FE_SLACK][96], rowoff [B + 1], info dict, and the tables of
        k_identity_prefix: prefix [B * 296 + FE_SLACK], counts [B + FE_SLACK]"""
        signals, wav_lens = np.ascontiguousarray(signals, np.float32), np.ascontiguousarray(wav_lens, np.float32)
        B = signals.shape[0]
        assert signals.shape == (B, 80000) and wav_lens.shape == (B,)
        feats = np.zeros((int(rows_all) + FE_SLACK, 96), np.float32)
        rowoff, info = np.full(B + 1, -1, np.int32), np.zeros(4, np.int64)
        prefix, counts = np.zeros(B * 296 + FE_SLACK, np.int32), np.zeros(B + FE_SLACK, np.int32)
        self._chk(lib().sd_test_frontend_signals(self._h, _ptr(signals), _ptr(wav_lens), B, int(bool(skip_dead_rows)), int(icanary), canary, _ptr(prefix),
                                                 _ptr(counts), _ptr(feats), feats.shape[0], _ptr(rowoff), _ptr(info)))
        return feats, rowoff, dict(zip(("n_active", "rows_all", "grid", "num_cu"), (int(v) for v in info))), prefix, counts

    # ---- the kernels behind the two networks alone (sdhip_test.h); every array comes back WHOLE, its BE_SLACK units included
    def binarize_case(self, seg, want=("bin", "masks", "nact"), fcanary=-7776.0, icanary=-7776):
        """sd_test_binarize: seg [chunks][293][3] -> dict of the arrays in `want`: bin [(chunks + BE_SLACK)][293][3] uint8, masks [(chunks + BE_SLACK) * 3][293],
        nact [(chunks + BE_SLACK) * 3]"""
        seg = np.ascontiguousarray(seg, np.float32)
        ck = seg.shape[0]
        assert seg.shape == (ck, 293, 3)
        out = {}
        if "bin" in want:
            out["bin"] = np.zeros((ck + BE_SLACK, 293, 3), np.uint8)
        if "masks" in want:
            out["masks"] = np.zeros(((ck + BE_SLACK) * 3, 293), np.float32)
        if "nact" in want:
            out["nact"] = np.zeros((ck + BE_SLACK) * 3, np.int32)
        p = lambda k: _ptr(out[k]) if k in out else None
        self._chk(lib().sd_test_binarize(self._h, _ptr(seg), ck, fcanary, icanary, p("bin"), p("masks"), p("nact")))
        return out

    def count_case(self, binarized, want_avg=True, fcanary=-7776.0, icanary=-7776):
        """sd_test_count: binarized [chunks][293][3] uint8 -> count [frames + BE_SLACK] int32, avg (or None) [frames + BE_SLACK] float64"""
        b = np.ascontiguousarray(binarized, np.uint8)
        ck = b.shape[0]
        assert b.shape == (ck, 293, 3)
        nf = int(lib().sd_count_frames(ck))
        cnt = np.zeros(nf + BE_SLACK, np.int32)
        avg = np.zeros(nf + BE_SLACK, np.float64) if want_avg else None
        self._chk(lib().sd_test_count(self._h, _ptr(b), ck, fcanary, icanary, _ptr(cnt), _ptr(avg) if want_avg else None))
        return cnt, avg

    def gather_normalize_case(self, X, tidx, want_xout=True, fcanary=-7776.0):
        """sd_test_gather_normalize: X [rows][d] float64, tidx [N] -> xout (or None), xn [N + BE_SLACK][d]"""
        X, tidx = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(tidx, np.int32)
        rows, d = X.shape
        N = len(tidx)
        xn = np.zeros((N + BE_SLACK, d), np.float64)
        xo = np.zeros((N + BE_SLACK, d), np.float64) if want_xout else None
        self._chk(lib().sd_test_gather_normalize(self._h, _ptr(X), rows, _ptr(tidx), N, d, fcanary, _ptr(xo) if want_xout else None, _ptr(xn)))
        return xo, xn

    def cluster_means_case(self, X, order, off, fcanary=-7776.0):
        """sd_test_cluster_means: X [rows][d] float64, order [off[-1]], off [nl + 1] -> cen [nl + BE_SLACK][d]"""
        X, order, off = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(order, np.int32), np.ascontiguousarray(off, np.int32)
        rows, d = X.shape
        nl = len(off) - 1
        assert len(order) == off[-1]
        cen = np.zeros((nl + BE_SLACK, d), np.float64)
        self._chk(lib().sd_test_cluster_means(self._h, _ptr(X), rows, d, _ptr(order), _ptr(off), nl, fcanary, _ptr(cen)))
        return cen

    def assign_case(self, E, cen, want_soft=True, want_best=True, fcanary=-7776.0, icanary=-7776):
        """sd_test_assign: E [M][d], cen [K][d] float64 -> hard [M + BE_SLACK], err [1 + BE_SLACK], soft [M + BE_SLACK][K] or None, best [M + BE_SLACK] or None"""
        E, cen = np.ascontiguousarray(E, np.float64), np.ascontiguousarray(cen, np.float64)
        (M, d), K = E.shape, cen.shape[0]
        assert cen.shape == (K, d)
        hard, err = np.zeros(M + BE_SLACK, np.int32), np.zeros(1 + BE_SLACK, np.int32)
        soft = np.zeros((M + BE_SLACK, K), np.float64) if want_soft else None
        best = np.zeros(M + BE_SLACK, np.float64) if want_best else None
        self._chk(lib().sd_test_assign(self._h, _ptr(E), M, d, _ptr(cen), K, fcanary, icanary, _ptr(hard), _ptr(err), _ptr(soft) if want_soft else None,
                                       _ptr(best) if want_best else None))
        return hard, err, soft, best

    def constrained_argmax_case(self, soft, fill, icanary=-7776):
        """sd_test_constrained_argmax: soft [chunks][3][K] float64, fill = what NaN scores become -> hard [(chunks + BE_SLACK)][3]"""
        soft = np.ascontiguousarray(soft, np.float64)
        ck, S, K = soft.shape
        assert S == 3
        hard = np.zeros((ck + BE_SLACK, 3), np.int32)
        self._chk(lib().sd_test_constrained_argmax(self._h, _ptr(soft), ck, K, float(fill), icanary, _ptr(hard)))
        return hard

    def activations_case(self, seg, hard, K, nact, fcanary=-7776.0):
        """sd_test_activations: seg [chunks][293][3] float32, hard [chunks][3], nact = the frames the caller expects -> act [nact + BE_SLACK][K]"""
        seg, hard = np.ascontiguousarray(seg, np.float32), np.ascontiguousarray(hard, np.int32)
        ck = seg.shape[0]
        assert seg.shape == (ck, 293, 3) and hard.shape == (ck, 3)
        act, n = np.zeros((int(nact) + BE_SLACK, K), np.float64), C.c_int64(0)
        self._chk(lib().sd_test_activations(self._h, _ptr(seg), _ptr(hard), ck, K, fcanary, _ptr(act), act.size, C.byref(n)))
        assert n.value == nact
        return act

    def topk_case(self, act, count, ar0, cr0, rows, crow):
        """sd_test_topk: act [act_rows][K] float64, count [n_count] int32 -> binary [rows + BE_SLACK][K] uint8 (slack: BE_BCANARY)"""
        act, count = np.ascontiguousarray(act, np.float64), np.ascontiguousarray(count, np.int32)
        ar, K = act.shape
        out = np.zeros((max(int(rows), 0) + BE_SLACK, K), np.uint8)
        self._chk(lib().sd_test_topk(self._h, _ptr(act), ar, _ptr(count) if len(count) else None, len(count), int(ar0), int(cr0), int(rows), int(crow), K, _ptr(out)))
        return out

    def assign_cuts_case(self, E, cen, coff, slot, n_slots, nact, fcanary=-7776.0, icanary=-7776):
        """sd_test_assign_cuts: E [M][d], cen [coff[-1]][d], coff [Tn + 1], slot [Tn], nact [M] -> m2 [coff[-1] + BE_SLACK], hard [n_slots * M + BE_SLACK],
        best [Tn * M + BE_SLACK], err [1 + BE_SLACK]"""
        E, cen = np.ascontiguousarray(E, np.float64), np.ascontiguousarray(cen, np.float64)
        coff, slot, nact = (np.ascontiguousarray(a, np.int32) for a in (coff, slot, nact))
        (M, d), Tn = E.shape, len(slot)
        assert cen.shape == (coff[-1], d) and len(coff) == Tn + 1 and len(nact) == M
        m2, hard = np.zeros(int(coff[-1]) + BE_SLACK, np.float64), np.zeros(n_slots * M + BE_SLACK, np.int32)
        best, err = np.zeros(Tn * M + BE_SLACK, np.float64), np.zeros(1 + BE_SLACK, np.int32)
        self._chk(lib().sd_test_assign_cuts(self._h, _ptr(E), M, d, _ptr(cen), _ptr(coff), _ptr(slot), Tn, int(n_slots), _ptr(nact), fcanary, icanary,
                                            _ptr(m2), _ptr(hard), _ptr(best), _ptr(err)))
        return m2, hard, best, err

    def recon_cuts_case(self, seg, hard, koff, nact, count, ar0, cr0, rows, crow, act_in=None, fcanary=-7776.0):
        """sd_test_recon_cuts: seg [chunks][293][3], hard [Tg][chunks * 3], koff [Tg + 1], nact = the frames the caller expects, count [n_count] ->
        act [nact * koff[-1] + BE_SLACK] float64, binary [rows * koff[-1] + BE_SLACK] uint8; act_in: the table k_topk_cuts reads instead of act"""
        seg, hard = np.ascontiguousarray(seg, np.float32), np.ascontiguousarray(hard, np.int32)
        koff, count = np.ascontiguousarray(koff, np.int32), np.ascontiguousarray(count, np.int32)
        ck, Tg, sumK = seg.shape[0], len(koff) - 1, int(koff[-1])
        assert seg.shape == (ck, 293, 3) and hard.shape == (Tg, ck * 3)
        act, binary, n = np.zeros(int(nact) * sumK + BE_SLACK, np.float64), np.zeros(max(int(rows), 0) * sumK + BE_SLACK, np.uint8), C.c_int64(0)
        if act_in is not None:
            act_in = np.ascontiguousarray(act_in, np.float64)
            assert act_in.size == int(nact) * sumK
        self._chk(lib().sd_test_recon_cuts(self._h, _ptr(seg), _ptr(hard), ck, _ptr(koff), Tg, _ptr(act_in) if act_in is not None else None,
                                           _ptr(count) if len(count) else None, len(count), int(ar0), int(cr0), int(rows), int(crow), fcanary, _ptr(act), act.size,
                                           _ptr(binary), C.byref(n)))
        assert n.value == nact
        return act, binary

    def pcm_to_f32_case(self, pcm, fcanary=-7776.0):
        """sd_test_pcm_to_f32: pcm [n] int16 -> [n + 512 + BE_SLACK] float32: the samples, SD_WAV_PAD zeros, the canary"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        out = np.zeros(len(pcm) + 512 + BE_SLACK, np.float32)
        self._chk(lib().sd_test_pcm_to_f32(self._h, _ptr(pcm), len(pcm), fcanary, _ptr(out)))
        return out

    def f32_to_f64_case(self, a, fcanary=-7776.0):
        """sd_test_f32_to_f64: a [n] float32 -> [n + BE_SLACK] float64"""
        a = np.ascontiguousarray(a, np.float32)
        out = np.zeros(len(a) + BE_SLACK, np.float64)
        self._chk(lib().sd_test_f32_to_f64(self._h, _ptr(a), len(a), fcanary, _ptr(out)))
        return out

    def mark_inactive_case(self, hard, nact, icanary=-7776):
        """sd_test_mark_inactive: hard [n], nact [n] int32 -> [n + BE_SLACK] int32"""
        hard, nact = np.ascontiguousarray(hard, np.int32), np.ascontiguousarray(nact, np.int32)
        assert hard.shape == nact.shape and hard.ndim == 1
        out = np.zeros(len(hard) + BE_SLACK, np.int32)
        self._chk(lib().sd_test_mark_inactive(self._h, _ptr(hard), _ptr(nact), len(hard), icanary, _ptr(out)))
        return out

    # ---- the kernels in front of the networks (sd_test_* of include/sdhip_test.h, csrc/input_test.hip); IN_SLACK units of canary behind every output
    def resample_case(self, x, in_sr, out_sr=16000, n_out=-1, want_taps=True, canary=-7776.0):
        """sd_test_resample: x [n] float32 -> y [n_out + IN_SLACK] float32 and, with want_taps, the context's tap table [2J + 1][L] (else None)"""
        x = np.ascontiguousarray(x, np.float32)
        full = int(lib().sd_resample_len(len(x), int(in_sr), int(out_sr)))
        no = full if n_out < 0 else int(n_out)
        y = np.zeros(max(no, 0) + IN_SLACK, np.float32)
        taps = None
        if want_taps:
            g = math.gcd(int(in_sr), int(out_sr))
            Lr, Mr = out_sr // g, in_sr // g
            J = int(np.floor(64.0 / (2.0 * (0.95 / (2.0 * max(Lr, Mr)))) / Lr)) + 1
            taps = np.zeros((2 * J + 1, Lr), np.float32)
        self._chk(lib().sd_test_resample(self._h, _ptr(x), len(x), int(in_sr), int(out_sr), int(n_out), canary, _ptr(y),
                                         _ptr(taps) if want_taps else None, taps.size if want_taps else 0))
        return y, taps

    def resample_jobs_case(self, rows, x, arena, canary=-7776.0, refused=False):
        """sd_test_resample_jobs: rows = (in_sr, pad, first, held, n_limit, m_first, count, x_off, dst_off) per row, x the shared inputs -> the arena
        [arena + IN_SLACK] float32.  refused = True: resample_jobs must refuse the table with SD_ERR_ARG, and the arena comes back all the same."""
        tab = np.zeros(len(rows), np.dtype([("in_sr", np.int32), ("pad", np.int32)] + [(k, np.int64) for k in ("first", "held", "n_limit", "m_first", "count", "x_off", "dst_off")]))
        for i, r in enumerate(rows):
            tab[i] = tuple(int(v) for v in r)
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros(int(arena) + IN_SLACK, np.float32)
        rc = lib().sd_test_resample_jobs(self._h, _ptr(tab), len(rows), _ptr(x), len(x), int(arena), canary, _ptr(out))
        if refused:
            assert rc == 1, rc                       # SD_ERR_ARG
            return out
        self._chk(rc)
        return out

    def group_copy_case(self, which, src, rows, dst_len, canary=-7776.0):
        """sd_test_group_copy: which 0 k_group_append (src int16 or float32), 1 k_group_scatter, 2 k_group_tail_move, 3 k_tail_move; rows [R][4] =
        (src_off, dst_off, len, room) -> [dst_len + IN_SLACK] float32"""
        src = np.ascontiguousarray(src)
        assert src.dtype in (np.float32, np.int16) and (src.dtype == np.float32 or which == 0)
        rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 4)
        out = np.zeros(int(dst_len) + IN_SLACK, np.float32)
        self._chk(lib().sd_test_group_copy(self._h, int(which), int(src.dtype == np.float32), _ptr(src), len(src), _ptr(rows), len(rows), int(dst_len), canary, _ptr(out)))
        return out

    def many_pack_case(self, src, rows, dst_len, canary=-7776.0):
        """sd_test_many_pack: src int16 or float32, rows [R][4] = (src_off or -1, n, base, len) -> [dst_len + IN_SLACK] float32"""
        src = np.ascontiguousarray(src)
        assert src.dtype in (np.float32, np.int16)
        rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 4)
        out = np.zeros(int(dst_len) + IN_SLACK, np.float32)
        self._chk(lib().sd_test_many_pack(self._h, int(src.dtype == np.float32), _ptr(src), len(src), _ptr(rows), len(rows), int(dst_len), canary, _ptr(out)))
        return out

    def many_ingest_case(self, rows, src, dst_len, canary=-7776.0, refused=False):
        """sd_test_many_ingest (include/sdhip_ingest_test.h): rows [R][8] = (encoding, channels, channel, sample_rate, n, src_off in bytes or -1, base, len),
        src = the bytes of all sources -> [dst_len + IN_SLACK] float32.  refused = True: the hook must refuse the table with SD_ERR_ARG before any launch."""
        src = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
        rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 8)
        out = np.zeros(int(dst_len) + IN_SLACK, np.float32)
        rc = lib().sd_test_many_ingest(self._h, _ptr(rows), len(rows), _ptr(src) if src.size else None, src.size, int(dst_len), canary, _ptr(out))
        if refused:
            assert rc == 1, rc                       # SD_ERR_ARG
            return out
        self._chk(rc)
        return out

    def group_ingest_case(self, rows, src, dst_len, canary=-7776.0, refused=False):
        """sd_test_group_ingest (include/sdhip_stream_ingest_test.h): rows [R][7] = (encoding, channels, channel, n, src_off in bytes, dst_off, room),
        src = the bytes of all sources -> [dst_len + IN_SLACK] float32.  refused = True: the hook must refuse the table with SD_ERR_ARG before any launch."""
        src = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
        rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 7)
        out = np.zeros(int(dst_len) + IN_SLACK, np.float32)
        rc = lib().sd_test_group_ingest(self._h, _ptr(rows), len(rows), _ptr(src) if src.size else None, src.size, int(dst_len), canary, _ptr(out))
        if refused:
            assert rc == 1, rc                       # SD_ERR_ARG
            return out
        self._chk(rc)
        return out

    def many_gap_masks_case(self, gaps, total_chunks, canary=-7776.0):
        """sd_test_many_gap_masks: gaps [G][2] = (first, count) -> [(total_chunks + IN_SLACK) * 3][293] float32"""
        gaps = np.ascontiguousarray(gaps, np.int64).reshape(-1, 2)
        out = np.zeros(((int(total_chunks) + IN_SLACK) * 3, 293), np.float32)
        self._chk(lib().sd_test_many_gap_masks(self._h, _ptr(gaps), len(gaps), int(total_chunks), canary, _ptr(out)))
        return out

    def weight_forms_case(self, w, cin, form, canary=0xC0DE):
        """sd_test_weight_forms: w [K][Cout][CinPad] float32; form 0: the fp16 planes [2][K][Cout][roundup64(cin)], form 1: the split form of
        sd_test_pack_split_weights -> (uint16 bit patterns with IN_SLACK canaries behind them, inverse scale)"""
        w = np.ascontiguousarray(w, np.float32)
        K, Cout, CinPad = w.shape
        halves = 2 * K * Cout * (CinPad if form else (cin + 63) // 64 * 64)
        out = np.zeros(halves + IN_SLACK, np.uint16)
        inv = C.c_float(0.0)
        self._chk(lib().sd_test_weight_forms(self._h, _ptr(w), K, Cout, CinPad, int(cin), int(form), canary, _ptr(out), out.size, C.byref(inv)))
        return out, np.float32(inv.value)

    def read_ws(self, name, dtype, count, offset=0):
        """test hook: `count` elements of the named device workspace"""
        out = np.zeros(count, dtype)
        self._chk(lib().sd_debug_read_ws(self._h, name.encode(), offset, _ptr(out), out.nbytes))
        return out

    def reset_stats(self):
        lib().sd_reset_stats(self._h)
