// main.cpp -- the `speakerDiarizer` command line, same surface as the reference's main()
// (sd.cpp:3415-3442):   speakerDiarizer <segment model> <embedding model> <16 kHz mono wav>
// prints the per-stage timings and, between two 52-dash rules, one line per turn:
//   [start -- end] --> Speaker_N
// Model files are the reference's ONNX files or .sdw weight packs (tools/make_weights.py); the
// whole path runs on the GPU through the C ABI of libsdhip.so.
//
// Extras after the three positional arguments (the reference has none):
//   --gpus N        shard the recording over N GPUs of this node: the launcher fork()s one
//                   process per GPU BEFORE anything touches HIP, rank 0 mints the RCCL rendezvous id and
//                   passes it to the others through pipes created before the fork; turns are printed by rank 0
//   --rttm FILE     also write the turns as RTTM
//   --precision P   f32 (default: f32 MFMA, the reference's ORT precision) | f16 (fp16 ECAPA layers, BASELINE configs[4]) | x3 (f32 tensors, both
//                   MFMA operands split into hi + lo fp16 halves in the ECAPA conv layers and PyanNet's LSTM: f32-grade results from the fp16 matrix
//                   pipe) = sd_set_option "ecapa_precision"; PyanNet's LSTM follows ("seg_precision" is left at auto for f16, set to 3 for x3: the same thing)
//   --resample      a wav whose sample rate is not 16 000 Hz is resampled on the GPU first (sd_resample; the dormant Resampler of the reference,
//                   frontend/resampler.cc:19-36).  WITHOUT it such a file is refused: the reference reads the rate and ignores it (sd.cpp:2940-2942),
//                   i.e. silently diarizes at the wrong speed
//   --assume-16k    the reference's own behaviour on such a file: the samples are processed as if they were 16 kHz whatever the header says
//                   (parity runs on off-rate files; SD_WAV_ASSUME_16K)
//   --downmix       average the channels of a multi-channel wav first (default: the reference's interleaved read, wav.h:95-97)
//   --dump-steps DIR [--dump-level 2]   the reference's WRITE_DATA switch: DIR/cpp_<item>.txt for the items of script/verifyEveryStepResult.py
//                   (sd_set_dump_dir; DIR = /tmp is what that script reads); single-GPU runs
//   --clustering-method NAME, --clustering-threshold X, --min-cluster-size N   the three hyper-parameters of clustering/Clustering.py:251-276
//                   (NAME: single | complete | average | centroid | median | ward | weighted; X in 0..2; N >= 1) = sd_set_option "clustering_method" /
//                   "min_cluster_size" and sd_set_option_f64 "clustering_threshold"; defaults are the reference's constants (centroid, 0.7153814, 15).
//                   A bad value is a usage error (exit 2) before anything touches the GPU
//   --max-num-embeddings N, --clustering-seed S   cluster a sample of at most N train rows and assign every row (BaseClustering.max_num_embeddings,
//                   Clustering.py:12, 69-76; N >= 1, or -1 = every row) = sd_set_option "max_num_embeddings"; S (any 64-bit integer, default 0) picks the
//                   sample = "clustering_seed".  A bad value is a usage error (exit 2) before anything touches the GPU
//   --activity speech|overlap   regions of speech / of overlapped speech from the segmentation network alone (sd_activity_wav: pyannote's
//                   VoiceActivityDetection / OverlappedSpeechDetection on the reference's aggregate + to_annotation, sd.cpp:1167-1311 / 2852-2935) instead of
//                   speaker turns: lines [start -- end] --> SPEECH or OVERLAP; --rttm writes them as SPEAKER_00 / SPEAKER_01.  With it
//                   --activity-onset X, --activity-offset X (in [0, 1], default 0.5), --activity-min-on S, --activity-min-off S (seconds >= 0, default 0)
//                   and --activity-hamming (Hamming-weighted aggregation) = the "activity_*" options.  A bad value is a usage error (exit 2) before
//                   anything touches the GPU; single-GPU only (--gpus N is refused)
//   --stream SECONDS [--stream-updates]   feed the recording through an sd_stream in pieces of SECONDS (> 0) as if it were still arriving: both networks run once
//                   per chunk as the audio comes in, the final turns are those of the run without the flag, bit for bit.  --stream-updates also prints,
//                   after each piece, "== <seconds pushed> s, <sealed>/<total> chunks" and the turns so far.  With - as the wav path, headerless s16le
//                   16 kHz mono samples are read from stdin until end of file (needs --stream).  Single GPU; not with --activity or --dump-steps
//   --stream-rate HZ   with --stream and - : the samples on stdin are headerless s16le at HZ (an integer > 0), resampled inside the stream
//                   (sd_stream_set_input_rate; 16000 = as without the flag); SECONDS are seconds of audio; sd_stream_end_input at end of file, before the
//                   final turns.  The "== N s" header of a --stream-updates block counts the 16 kHz samples the stream holds so far, which trail the
//                   audio pushed by the filter wing (8.5 ms at 8 kHz) until the end of the input.  Without
//                   --stream, with a wav file instead of -, or with another value: usage error (exit 2)
//   --stream-encoding s16|f32|mulaw|alaw   --stream-channels N   --stream-channel C|mean   with --stream and - : stdin holds headerless interleaved
//                   frames of N elements (default 1) in that encoding (default s16; little-endian int16 or float, or one G.711 code per byte), of
//                   which the stream takes channel C (default 0) or their mean (sd_stream_set_input_format, sd_stream_push_audio), at --stream-rate HZ
//                   or 16 kHz; a piece is SECONDS x rate frames.  Bytes of a partial frame carry over to the next read; a partial frame at end of
//                   file is dropped with a line on stderr.  Without --stream and -, or with a bad value (N < 1, C outside 0 .. N-1): usage error (exit 2)
//   --stream-window SECONDS   with --stream: a sliding window (sd_stream_set_window with ceil(SECONDS / 16) blocks of 32 chunks): after every piece that
//                   seals a block the stream forgets all but that many; the turns are those of the audio still held, printed with absolute times
//                   (t + sd_stream_origin / 16000); the header of a --stream-updates block still gives the seconds pushed, its chunk counts are those of the
//                   audio held.  Without --stream, or with a value that is not a number of seconds > 0: usage error (exit 2)
//   --stream-roster   with --stream: a speaker roster on the stream (sd_roster_open, sd_stream_set_roster): every printed label -- in every --stream-updates
//                   block as well -- is a roster id, which means the same person from one update to the next and, with --stream-window, for a talker
//                   who left the window and came back.  Without --stream: usage error (exit 2); refused with --speakers and --relabel, which name
//                   and renumber raw labels
//   --speakers FILE [--speakers-threshold X]   after the diarization, match the centroids of the job's clusters (sd_last_speakers) against the voiceprints of
//                   FILE (sd_read_voiceprints, sd_match_speakers): a matched cluster prints as [start -- end] --> NAME and goes into the RTTM under its name, an
//                   unmatched one prints as without the flag.  X in [0, 2] = the largest cosine distance that still matches (option "speaker_match_threshold").
//                   Works with --stream; refused with --activity and with --gpus N > 1
//   --speakers FILE --enrolled [--speakers-threshold X]   enrol the voiceprints of FILE BEFORE the job (sd_set_enrolled): the clustering itself claims the
//                   embeddings within X of a voiceprint for that person, clusters the rest and prints / writes the names sd_last_enrolled gives -- no
//                   matching afterwards.  With --stream a label means the same person in every update (--stream-updates prints the names too).
//                   Refused with --enroll, --activity, --dump-steps and --gpus N > 1
//   --enroll NAME --speakers FILE [--enroll-span START END]...   no diarization: the voiceprint of the wav -- all of it, or the given spans in seconds --
//                   (sd_voiceprint_wav) replaces or is appended as NAME in FILE (created when absent); prints "enrolled NAME from N windows".
//                   A bad value of any of these is a usage error (exit 2) before anything touches the GPU
//   --many LIST     instead of the wav argument: LIST names one wav file per line (empty lines and lines that start with # are skipped); all of them go
//                   through the two networks together (sd_diarize_many_audio) and each gets the turns of a run of its own, bit for bit.  Every file is read
//                   with the --resample / --downmix / --assume-16k rules of the single-file path.  16-bit PCM, mu-law (format tag 7) and A-law (tag 6)
//                   files of any rate and channel count go to the GPU as they are and are decoded, downmixed and resampled there while the packed
//                   waveform is filled -- no sd_resample per file; a multi-channel G.711 file needs --downmix and is refused without it, an off-rate
//                   file without --resample is refused as in the single-file path.  8- and 32-bit PCM, and multi-channel PCM without --downmix (read
//                   as the reference reads it), go through the host readers into the same call.  Output: a line "== <path>" and that file's turns, in
//                   list order; a file that cannot be read, is refused or is too short gets "== <path>: <message>" and the exit status is 1.
//                   --rttm DIR writes DIR/<file name without .wav>.rttm per recording; --speakers (with or without --enrolled) and --relabel work per
//                   recording.  Refused with --gpus N > 1, --stream, --activity, --dump-steps and --enroll
//   --score REF.rttm [--collar X] [--skip-overlap] [--uem-from-ref]   after the diarization, one more line on stderr: the diarization error rate of the turns
//                   against the SPEAKER lines of REF.rttm (sd_read_rttm, sd_der: the rule of pyannote.metrics' DiarizationErrorRate),
//                   "DER d (missed m, false alarm f, confusion c, total t s)".  X = the collar in seconds (half on each side of every reference boundary),
//                   --skip-overlap leaves reference overlap unscored, --uem-from-ref scores the time from the first reference start to the last reference end only
//   --tune REF.rttm --thresholds LO:HI:N [--min-cluster-sizes a,b,...]   no single diarization: one cut object (sd_cut_open_wav: both networks and the linkage
//                   once) and the grid of N thresholds from LO to HI (N = 1: LO) times the sizes, thresholds outermost, in one sd_cut_turns_many; one line
//                   "threshold T min_cluster_size M speakers K DER d (...)" per point and "best threshold T min_cluster_size M DER d", the first minimum in
//                   grid order.  The scoring flags of --score apply.  A bad grid or an unreadable REF.rttm is a usage error (exit 2) before anything touches
//                   the GPU.  Both are single-GPU, whole-file options: refused with --gpus N > 1, --stream, --activity, --many, --enroll and each other;
//                   --tune also with --enrolled and --dump-steps
//   --relabel       stdout / RTTM labels renumbered the way pyannote.audio names its output (the clusters that occur,
//                   sorted by their string, become 0, 1, ... = SPEAKER_00, SPEAKER_01, ...); default = raw cluster ids (sd.cpp:3439)
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <ctime>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <csignal>
#include <sys/wait.h>
#include <unistd.h>
#include "sdhip.h"
#include "many_plan.h"
#include "wav_file.h"

struct Args { const char* seg = nullptr; const char* emb = nullptr; const char* wav = nullptr; const char* rttm = nullptr; int gpus = 1; bool relabel = false; int precision = 0; int wav_flags = 0; const char* dump_dir = nullptr; int dump_level = 1;
              int cl_method = -1; double cl_threshold = -1.0; long long cl_min_size = -1;         // -1: leave the library's default
              long long cl_max_num = 0, cl_seed = 0; bool cl_seed_set = false;                    // --max-num-embeddings (0: not given), --clustering-seed
              long long stream_window = -1;                                                       // --stream-window: blocks kept (-1: no window)
              int activity = -1; double act[4] = {-1.0, -1.0, -1.0, -1.0}; bool act_hamming = false;      // --activity: SD_ACTIVITY_*; onset, offset, min on, min off (-1: default)
              long long stream_piece = 0; bool stream_updates = false;         // --stream: samples per piece (0: off)
              bool stream_roster = false;                                      // --stream-roster: the labels are roster ids
              long long stream_rate = 0; double stream_sec = 0.0;              // --stream-rate: the sample rate of stdin (0: 16 000); --stream's SECONDS as given
              bool stream_fmt = false;                                         // --stream-encoding / -channels / -channel: stdin holds frames in that format
              int stream_enc = SD_ENC_S16; long long stream_channels = 1, stream_channel = 0;
              const char* speakers = nullptr; double speakers_threshold = -1.0; const char* enroll = nullptr; std::vector<sd_turn> enroll_spans; bool enrolled = false;
              const char* many = nullptr;         // --speakers FILE, its threshold (-1: default), --enroll NAME and its spans
              const char* score = nullptr; const char* tune = nullptr; double collar = 0.0; bool skip_overlap = false, uem_from_ref = false;      // --score / --tune REF.rttm and how to score
              std::vector<double> thresholds; std::vector<long long> min_sizes;      // --tune: the grid
              std::vector<sd_turn> ref; };        // the turns of REF.rttm, read before anything touches the GPU

// --score / --tune: the error rate of `turns` against a.ref by the command line's scoring flags, as the text behind "DER "; false (message printed) on a failure
static bool score_turns(const Args& a, const sd_turn* turns, int64_t nt, sd_der_result& r, char* text, size_t cap)
{
    sd_turn uem{0.0, 0.0, 0, 0};
    if (a.uem_from_ref && !a.ref.empty()) {
        uem.start = a.ref[0].start; uem.end = a.ref[0].end;
        for (const sd_turn& t : a.ref) { if (t.start < uem.start) uem.start = t.start; if (t.end > uem.end) uem.end = t.end; }
    }
    if (sd_der(a.ref.data(), (int64_t)a.ref.size(), turns, nt, a.uem_from_ref ? &uem : nullptr, a.uem_from_ref ? 1 : 0, a.collar, a.skip_overlap ? 1 : 0, &r, nullptr, 0, nullptr) != SD_OK) {
        fprintf(stderr, "scoring failed: %s\n", sd_score_error());
        return false;
    }
    snprintf(text, cap, "%.17g (missed %.17g, false alarm %.17g, confusion %.17g, total %.17g s)", r.der, r.missed, r.false_alarm, r.confusion, r.total);
    return true;
}

// the clustering hyper-parameters the command line set; false (message printed) on a refusal
static bool apply_clustering(sd_ctx* ctx, const Args& a)
{
    if (a.cl_method >= 0 && sd_set_option(ctx, "clustering_method", a.cl_method) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return false; }
    if (a.cl_threshold >= 0.0 && sd_set_option_f64(ctx, "clustering_threshold", a.cl_threshold) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return false; }
    if (a.cl_min_size >= 0 && sd_set_option(ctx, "min_cluster_size", a.cl_min_size) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return false; }
    if (a.cl_max_num != 0 && sd_set_option(ctx, "max_num_embeddings", a.cl_max_num) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return false; }
    if (a.cl_seed_set && sd_set_option(ctx, "clustering_seed", a.cl_seed) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return false; }
    return true;
}

// the context of a run: created on `device`, --precision and the clustering hyper-parameters set.  Null on a failure: the message is printed (behind
// `prefix`: run_rank's "rank N: ") and what was created is destroyed
static sd_ctx* open_context(const Args& a, int device = 0, const char* prefix = "")
{
    sd_ctx* ctx = sd_create(a.seg, a.emb, device);
    if (!ctx) { fprintf(stderr, "%ssd_create failed: %s\n", prefix, sd_create_error()); return nullptr; }
    if ((a.precision && sd_set_option(ctx, "ecapa_precision", a.precision) != SD_OK) || (a.precision == 3 && sd_set_option(ctx, "seg_precision", 3) != SD_OK))
        fprintf(stderr, "%s%s\n", prefix, sd_last_error(ctx));
    else if (apply_clustering(ctx, a)) return ctx;
    sd_destroy(ctx);
    return nullptr;
}

static const char* const kActivityKeys[4] = {"activity_onset", "activity_offset", "activity_min_duration_on", "activity_min_duration_off"};
static bool apply_activity(sd_ctx* ctx, const Args& a)
{
    for (int q = 0; q < 4; ++q)
        if (a.act[q] >= 0.0 && sd_set_option_f64(ctx, kActivityKeys[q], a.act[q]) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return false; }
    if (a.act_hamming && sd_set_option(ctx, "activity_hamming", 1) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return false; }
    return true;
}

// a voiceprint file in memory (--speakers)
struct Gallery {
    char** names = nullptr; double* emb = nullptr; int64_t M = 0;
    ~Gallery() { sd_free_voiceprints(names, emb, M); }
    bool read(const char* path) { if (sd_read_voiceprints(path, &names, &emb, &M) == SD_OK) return true; fprintf(stderr, "%s\n", sd_voiceprints_error()); return false; }
};

// --speakers: names[k] = the name of the voiceprint that the centroid of raw label k matched, or null; false (message printed) on a failure
static bool match_clusters(sd_ctx* ctx, const Args& a, const Gallery& g, std::vector<const char*>& names)
{
    names.clear();
    int64_t K = 0;
    if (sd_last_speakers(ctx, nullptr, 0, &K, nullptr) != SD_OK) return false;
    names.assign((size_t)K, nullptr);
    if (K == 0 || g.M == 0) return true;
    if (a.speakers_threshold >= 0.0 && sd_set_option_f64(ctx, "speaker_match_threshold", a.speakers_threshold) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return false; }
    std::vector<int32_t> match((size_t)K);
    const int rc = sd_match_speakers(ctx, nullptr, K, g.emb, g.M, SD_EMB_DIM, NAN, match.data(), nullptr);
    if (rc != SD_OK) { fprintf(stderr, "matching against %s failed (%d): %s\n", a.speakers, rc, sd_last_error(ctx)); return false; }
    for (int64_t k = 0; k < K; ++k) if (match[(size_t)k] >= 0) names[(size_t)k] = g.names[match[(size_t)k]];
    return true;
}

// --speakers FILE --enrolled, before the job: the threshold, then the gallery; false (message printed) on a failure
static bool enrol_gallery(sd_ctx* ctx, const Args& a, const Gallery& g)
{
    if (a.speakers_threshold >= 0.0 && sd_set_option_f64(ctx, "speaker_match_threshold", a.speakers_threshold) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return false; }
    const int rc = sd_set_enrolled(ctx, g.emb, g.M, SD_EMB_DIM);
    if (rc != SD_OK) { fprintf(stderr, "enrolling %s failed (%d): %s\n", a.speakers, rc, sd_last_error(ctx)); return false; }
    return true;
}

// ... and after it: names[k] = the name of the voiceprint that raw label k stands for (sd_last_enrolled), or null
static bool enrolled_names(sd_ctx* ctx, const Gallery& g, std::vector<const char*>& names)
{
    names.clear();
    int64_t K = 0;
    if (sd_last_enrolled(ctx, nullptr, 0, &K) != SD_OK) return false;
    std::vector<int32_t> rows((size_t)K, -1);
    if (K > 0 && sd_last_enrolled(ctx, rows.data(), K, &K) != SD_OK) return false;
    names.assign((size_t)K, nullptr);
    for (int64_t k = 0; k < K; ++k) if (rows[(size_t)k] >= 0 && rows[(size_t)k] < g.M) names[(size_t)k] = g.names[rows[(size_t)k]];
    return true;
}

// --speakers, after a job: names[k] = the name raw label k of the last job goes by, or null; false (message printed) on a failure
static bool cluster_names(sd_ctx* ctx, const Args& a, const Gallery& g, std::vector<const char*>& names)
{
    return a.enrolled ? enrolled_names(ctx, g, names) : match_clusters(ctx, a, g, names);
}

// The turn lines of a block.  First the name of every turn by its raw label (names: null = none), then --relabel renumbers the labels, then the lines.
// turn_name: the name each turn was printed under, or null
static void print_turns(sd_turn* turns, int64_t nt, const Args& a, const std::vector<const char*>* names, std::vector<const char*>& turn_name)
{
    turn_name.assign((size_t)nt, nullptr);
    if (names) for (int64_t i = 0; i < nt; ++i) if (turns[i].label >= 0 && (size_t)turns[i].label < names->size()) turn_name[(size_t)i] = (*names)[(size_t)turns[i].label];
    if (a.relabel && a.activity < 0) sd_relabel_turns(turns, nt);
    char line[160];
    for (int64_t i = 0; i < nt; ++i) {
        if (turn_name[(size_t)i]) { printf("[%g -- %g] --> %s\n", turns[i].start, turns[i].end, turn_name[(size_t)i]); continue; }
        if (a.activity >= 0) snprintf(line, sizeof(line), "[%g -- %g] --> %s", turns[i].start, turns[i].end, turns[i].label == SD_ACTIVITY_OVERLAP ? "OVERLAP" : "SPEECH");
        else sd_format_turn(&turns[i], line, sizeof(line));
        printf("%s\n", line);
    }
}

// the name table of sd_write_rttm_named: names by the labels as they are behind print_turns
static std::vector<const char*> names_by_label(const sd_turn* turns, int64_t nt, const std::vector<const char*>& turn_name)
{
    std::vector<const char*> by_label;
    for (int64_t i = 0; i < nt; ++i) if (turns[i].label >= 0) { if ((size_t)turns[i].label >= by_label.size()) by_label.resize((size_t)turns[i].label + 1, nullptr); by_label[(size_t)turns[i].label] = turn_name[(size_t)i]; }
    return by_label;
}

static void print_block(sd_ctx* ctx, sd_turn* turns, int64_t nt, const Args& a, const double* ms_sum = nullptr, const std::vector<const char*>* names = nullptr)
{
    double ms[4];
    if (ms_sum) memcpy(ms, ms_sum, sizeof(ms)); else sd_stage_ms(ctx, ms);
    printf("-----------\nSegmenations time: %lldms\n", (long long)ms[0]);      // labels of sd.cpp:3028, 3110, 3231
    printf("-----------\nEmbedding time: %lldms\n", (long long)ms[1]);
    printf("-----------\nClustering time: %lldms\n", (long long)ms[2]);
    printf("\n----Summary----\n-----------\nTime cost: %lldms\n", (long long)ms[3]);
    printf("----------------------------------------------------\n");
    std::vector<const char*> turn_name;
    print_turns(turns, nt, a, names, turn_name);
    printf("----------------------------------------------------\n");
    if (a.rttm && names) {
        const std::vector<const char*> by_label = names_by_label(turns, nt, turn_name);
        sd_write_rttm_named(a.rttm, a.wav, turns, nt, nullptr, by_label.data(), (int64_t)by_label.size());
    }
    else if (a.rttm) sd_write_rttm(a.rttm, a.wav, turns, nt);
    fflush(stdout);
}

static double wall_ms()
{
    struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
static const bool g_trace = getenv("SD_TRACE_CREATE") != nullptr;     // start-up breakdown on stderr (tools/cold_start.py)
static double g_t_main = 0;
#define TRACE(what) do { if (g_trace) fprintf(stderr, "cli: +%.1f ms %s\n", wall_ms() - g_t_main, what); } while (0)

// --enroll: the voiceprint of the wav (of its spans) into the voiceprint file under a.enroll
static int run_enroll(const Args& a)
{
    Gallery g;
    if (access(a.speakers, F_OK) == 0 && !g.read(a.speakers)) return 1;      // an existing file must be a voiceprint file; an absent one is created
    sd_ctx* ctx = sd_create(nullptr, a.emb, 0);
    if (!ctx) { fprintf(stderr, "sd_create failed: %s\n", sd_create_error()); return 1; }
    if (a.precision && sd_set_option(ctx, "ecapa_precision", a.precision) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); sd_destroy(ctx); return 1; }
    double emb[SD_EMB_DIM]; int64_t nw = 0;
    const int rc = sd_voiceprint_wav(ctx, a.wav, a.wav_flags, a.enroll_spans.empty() ? nullptr : a.enroll_spans.data(), (int64_t)a.enroll_spans.size(), -1, emb, &nw);
    if (rc != SD_OK) { fprintf(stderr, "enrolment failed (%d): %s\n", rc, sd_last_error(ctx)); sd_destroy(ctx); return 1; }
    sd_destroy(ctx);
    std::vector<const char*> names; std::vector<double> all;
    bool replaced = false;
    for (int64_t i = 0; i < g.M; ++i) {
        names.push_back(g.names[i]);
        const bool same = strcmp(g.names[i], a.enroll) == 0;
        const double* src = same ? emb : g.emb + i * SD_EMB_DIM;
        all.insert(all.end(), src, src + SD_EMB_DIM);
        replaced |= same;
    }
    if (!replaced) { names.push_back(a.enroll); all.insert(all.end(), emb, emb + SD_EMB_DIM); }
    if (sd_write_voiceprints(a.speakers, names.data(), all.data(), (int64_t)names.size()) != SD_OK) { fprintf(stderr, "%s\n", sd_voiceprints_error()); return 1; }
    printf("enrolled %s from %lld windows\n", a.enroll, (long long)nw);
    return 0;
}

static int run_single(const Args& a)
{
    TRACE("run_single");
    Gallery g;
    if (a.speakers && !g.read(a.speakers)) return 1;
    sd_ctx* ctx = open_context(a);
    if (!ctx) return 1;
    TRACE("sd_create done");
    sd_turn* turns = nullptr; int64_t nt = 0;
    auto leave = [&](int rc) { sd_free_turns(turns); sd_destroy(ctx); return rc; };      // every way out gives back what it holds
    if (a.dump_dir && sd_set_dump_dir(ctx, a.dump_dir, a.dump_level) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return leave(1); }
    if (!apply_activity(ctx, a)) return leave(1);
    if (a.enrolled && !enrol_gallery(ctx, a, g)) return leave(1);
    const int rc = a.activity >= 0 ? sd_activity_wav(ctx, a.wav, a.wav_flags, a.activity, &turns, &nt)
                                   : sd_diarize_wav(ctx, a.wav, a.wav_flags, &turns, &nt);      // 8 / 16 / 32-bit PCM like wav.h:99-122; rate and channels checked
    if (rc != SD_OK) { fprintf(stderr, "%s failed (%d): %s\n", a.activity >= 0 ? "activity detection" : "diarization", rc, sd_last_error(ctx)); return leave(1); }
    TRACE("sd_diarize_wav done");
    char der_text[256]; sd_der_result der;
    if (a.score && !score_turns(a, turns, nt, der, der_text, sizeof(der_text))) return leave(1);      // on the raw labels, before --relabel
    std::vector<const char*> names;
    if (a.speakers && !cluster_names(ctx, a, g, names)) return leave(1);
    print_block(ctx, turns, nt, a, nullptr, a.speakers ? &names : nullptr);
    if (a.score) fprintf(stderr, "DER %s\n", der_text);
    const int done = leave(0);
    TRACE("sd_destroy done");
    return done;
}

// --tune: one cut object, the grid in one sd_cut_turns_many, every point scored against a.ref
static int run_tune(const Args& a)
{
    sd_ctx* ctx = open_context(a);
    if (!ctx) return 1;
    sd_cut* cut = nullptr;
    std::vector<sd_cut_spec> specs;
    for (double t : a.thresholds) for (long long m : a.min_sizes) specs.push_back(sd_cut_spec{t, (int32_t)m, 0});
    const int64_t T = (int64_t)specs.size();
    std::vector<sd_turn*> turns((size_t)T, nullptr);
    std::vector<int64_t> nt((size_t)T, 0);
    std::vector<int32_t> K((size_t)T, 0);
    auto leave = [&](int rc) { for (sd_turn* t : turns) sd_free_turns(t); sd_cut_close(cut); sd_destroy(ctx); return rc; };
    int rc = sd_cut_open_wav(ctx, a.wav, a.wav_flags, &cut);
    if (rc == SD_OK) rc = sd_cut_turns_many(cut, specs.data(), T, turns.data(), nt.data(), K.data());
    if (rc != SD_OK) { fprintf(stderr, "tuning failed (%d): %s\n", rc, sd_last_error(ctx)); return leave(1); }
    int64_t best = -1; double best_der = NAN;
    char text[256];
    for (int64_t i = 0; i < T; ++i) {
        sd_der_result r;
        if (!score_turns(a, turns[(size_t)i], nt[(size_t)i], r, text, sizeof(text))) return leave(1);
        printf("threshold %.17g min_cluster_size %d speakers %d DER %s\n", specs[(size_t)i].threshold, specs[(size_t)i].min_cluster_size ? specs[(size_t)i].min_cluster_size : 15, K[(size_t)i], text);
        if (best < 0 || (r.der == r.der && !(best_der <= r.der))) { best = i; best_der = r.der; }      // the first minimum in grid order
    }
    printf("best threshold %.17g min_cluster_size %d DER %.17g\n", specs[(size_t)best].threshold, specs[(size_t)best].min_cluster_size ? specs[(size_t)best].min_cluster_size : 15, best_der);
    return leave(0);
}

// ---- the off-rate samples of a file (WavLoad::F32_OFF_RATE) at 16 kHz: sd_resample, the kernel the wav entries of the library resample with
static int resample_16k(sd_ctx* ctx, const WavLoad& f, std::vector<float>& out)
{
    const int64_t cap = sd_resample_len(f.n, f.sr, 16000);
    out.assign((size_t)(cap > 0 ? cap : 1), 0.0f);
    int64_t no = 0;
    const int rc = sd_resample(ctx, f.f32, f.n, f.sr, 16000, out.data(), (int64_t)out.size(), &no);
    out.resize((size_t)(rc == SD_OK ? no : 0));
    return rc;
}

// ---- --many: the samples sd_diarize_wav would diarize (wav_load: same readers, same --resample / --downmix / --assume-16k rules) as host floats; 16-bit
// samples divided by 32768 here are the floats k_pcm_to_f32 makes of them (the division is exact)
static bool many_load(sd_ctx* ctx, const char* path, int flags, std::vector<float>& out, std::string& msg)
{
    WavLoad f;
    wav_load(path, flags, f);
    if (f.refused()) { msg = f.msg; return false; }
    if (f.kind == WavLoad::PCM16) { out.resize((size_t)f.n); for (int64_t i = 0; i < f.n; ++i) out[(size_t)i] = (float)f.pcm[i] * (1.0f / 32768.0f); }
    else if (f.kind == WavLoad::F32) out.assign(f.f32, f.f32 + f.n);
    else if (resample_16k(ctx, f, out) != SD_OK) { msg = std::string("resampling failed: ") + sd_last_error(ctx); return false; }
    return true;
}

// ---- --many: a file sd_read_wav_audio can describe -- 16-bit PCM, mu-law, A-law -- goes to sd_diarize_many_audio as it is: decoded, downmixed and resampled on
// the device while the pack is filled, no sd_resample per file.  true: desc / data are set (the caller frees data); false with an empty msg: not such a
// file, or multi-channel PCM without --downmix, whose "first n interleaved samples" reading stays many_load's; false with a msg: refused
static bool many_describe(const char* path, int flags, sd_audio& desc, void*& data, std::string& msg)
{
    data = nullptr;
    if (sd_read_wav_audio(path, &desc, &data) != SD_OK) return false;
    auto drop = [&]() { free(data); data = nullptr; return false; };
    const bool g711 = desc.encoding != SD_ENC_S16;
    if (desc.channels > 1 && !(flags & SD_WAV_DOWNMIX)) {
        if (g711) msg = std::to_string(desc.channels) + " channels of G.711; pass --downmix to diarize their mean (one channel of a file: sd_diarize_many_audio)";
        return drop();
    }
    if (desc.channels > 1) desc.channel = -1;
    if (flags & SD_WAV_ASSUME_16K) desc.sample_rate = 16000;
    if (desc.sample_rate != 16000 && !(flags & SD_WAV_RESAMPLE)) {
        if (g711) msg = "sample rate " + std::to_string(desc.sample_rate) + " Hz; the pipeline needs 16000 -- pass SD_WAV_RESAMPLE / --resample (or SD_WAV_ASSUME_16K / --assume-16k)";
        return drop();      // (a PCM file: many_load refuses it with wav_load's own line)
    }
    if (desc.n <= 0) { msg = "holds no samples"; return drop(); }
    return true;
}

static int run_many(const Args& a)
{
    std::vector<std::string> paths; std::string err;
    if (!many_read_list(a.many, paths, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    Gallery g;
    if (a.speakers && !g.read(a.speakers)) return 1;
    sd_ctx* ctx = open_context(a);
    if (!ctx) return 1;
    const size_t P = paths.size();
    std::vector<std::vector<float>> wav(P);
    std::vector<void*> raw(P, nullptr);
    auto leave = [&](int rc) { for (void* p : raw) free(p); sd_destroy(ctx); return rc; };
    if (a.enrolled && !enrol_gallery(ctx, a, g)) return leave(1);
    std::vector<std::string> msg(P);
    std::vector<sd_audio> rows; std::vector<int64_t> lens; std::vector<size_t> who;      // the files that were read
    for (size_t i = 0; i < P; ++i) {
        sd_audio d{};
        if (many_describe(paths[i].c_str(), a.wav_flags, d, raw[i], msg[i])) { rows.push_back(d); lens.push_back(sd_audio_len16(&d)); who.push_back(i); continue; }
        if (!msg[i].empty()) continue;
        if (many_load(ctx, paths[i].c_str(), a.wav_flags, wav[i], msg[i])) {      // the rest: 16 kHz mono floats from the host readers, in the same call
            if (wav[i].empty()) { msg[i] = "holds no samples"; continue; }
            rows.push_back(sd_audio{wav[i].data(), (int64_t)wav[i].size(), 16000, SD_ENC_F32, 1, 0}); lens.push_back((int64_t)wav[i].size()); who.push_back(i);
        }
    }
    const size_t R = rows.size();
    std::vector<sd_turn*> turns(R ? R : 1, nullptr); std::vector<int64_t> nt(R ? R : 1, 0); std::vector<int32_t> status(R ? R : 1, SD_OK);
    if (R > 0) {
        const int rc = sd_diarize_many_audio(ctx, rows.data(), (int64_t)R, turns.data(), nt.data(), status.data());
        if (rc != SD_OK) { fprintf(stderr, "diarization failed (%d): %s\n", rc, sd_last_error(ctx)); return leave(1); }
        double ms[4]; sd_stage_ms(ctx, ms);
        fprintf(stderr, "%zu recordings: segmentation %.1f ms, embedding %.1f ms, clustering %.1f ms, call %.1f ms\n", R, ms[0], ms[1], ms[2], ms[3]);
    }
    std::vector<size_t> slot(P, (size_t)-1);
    for (size_t r = 0; r < R; ++r) slot[who[r]] = r;
    int worst = 0;
    std::vector<std::string> stems;
    for (size_t i = 0; i < P; ++i) {
        const size_t r = slot[i];
        if (r != (size_t)-1 && status[r] == SD_ERR_SHORT) msg[i] = "audio of " + std::to_string(lens[r]) + " samples yields no chunk";
        else if (r != (size_t)-1 && status[r] != SD_OK) msg[i] = "diarization failed (" + std::to_string(status[r]) + ")";
        if (r == (size_t)-1 || status[r] != SD_OK) { printf("== %s: %s\n", paths[i].c_str(), msg[i].c_str()); worst = 1; continue; }
        printf("== %s\n", paths[i].c_str());
        std::vector<const char*> names, turn_name;
        const bool named = a.speakers && sd_many_select(ctx, (int64_t)r) == SD_OK && cluster_names(ctx, a, g, names);
        print_turns(turns[r], nt[r], a, named ? &names : nullptr, turn_name);
        if (a.rttm) {
            std::string stem = paths[i].substr(paths[i].find_last_of('/') == std::string::npos ? 0 : paths[i].find_last_of('/') + 1);
            if (stem.size() > 4 && stem.compare(stem.size() - 4, 4, ".wav") == 0) stem.resize(stem.size() - 4);
            for (const std::string& s : stems) if (s == stem) { stem += "_" + std::to_string(i); break; }      // the same file name twice in the list
            stems.push_back(stem);
            const std::string out = std::string(a.rttm) + "/" + stem + ".rttm";
            const std::vector<const char*> by_label = names_by_label(turns[r], nt[r], turn_name);
            const int rc = a.speakers ? sd_write_rttm_named(out.c_str(), paths[i].c_str(), turns[r], nt[r], nullptr, by_label.data(), (int64_t)by_label.size())
                                      : sd_write_rttm(out.c_str(), paths[i].c_str(), turns[r], nt[r]);
            if (rc != SD_OK) { fprintf(stderr, "cannot write %s\n", out.c_str()); worst = 1; }
        }
    }
    fflush(stdout);
    for (size_t r = 0; r < R; ++r) sd_free_turns(turns[r]);
    return leave(worst);
}

// ---- --stream: the recording goes through an sd_stream piece by piece
struct StreamRun {
    sd_ctx* ctx; sd_stream* st; const Args& a;
    double ms[4] = {0, 0, 0, 0};                    // stage times summed over every call of the run
    sd_turn* turns = nullptr; int64_t nt = 0;
    const Gallery* gal = nullptr;                   // --enrolled: the update blocks print the names too
    void bill() { double m[4]; sd_stage_ms(ctx, m); for (int q = 0; q < 4; ++q) ms[q] += m[q]; }
    // turns of what has been pushed; too little audio for a chunk is no turns yet, not a failure
    bool ask()
    {
        sd_free_turns(turns); turns = nullptr; nt = 0;
        const int rc = sd_stream_turns(st, &turns, &nt);
        if (rc == SD_ERR_SHORT) return true;
        if (rc != SD_OK) { fprintf(stderr, "diarization failed (%d): %s\n", rc, sd_last_error(ctx)); return false; }
        bill();
        int64_t origin = 0;                         // --stream-window: the stream's times count from the first sample it still holds
        sd_stream_origin(st, &origin);
        if (origin > 0) for (int64_t i = 0; i < nt; ++i) { turns[i].start += (double)origin / 16000.0; turns[i].end += (double)origin / 16000.0; }
        return true;
    }
    // one push call; a piece may take several (stdin arrives in smaller reads)
    bool part(int rc)
    {
        if (rc != SD_OK) { fprintf(stderr, "sd_stream_push failed (%d): %s\n", rc, sd_last_error(ctx)); return false; }
        bill();
        return true;
    }
    // a whole piece is in: the update block, if asked for
    bool piece_done()
    {
        if (!a.stream_updates) return true;
        if (!ask()) return false;
        int64_t n = 0, sealed = 0, total = 0;
        sd_stream_info(st, &n, &sealed, &total);
        int64_t origin = 0;                         // --stream-window: seconds pushed, not seconds held; the chunks are those the stream still holds
        sd_stream_origin(st, &origin);
        printf("== %g s, %lld/%lld chunks\n", (double)(origin + n) / SD_SAMPLE_RATE, (long long)sealed, (long long)total);
        std::vector<const char*> names, turn_name;
        print_turns(turns, nt, a, gal && enrolled_names(ctx, *gal, names) ? &names : nullptr, turn_name);
        fflush(stdout);
        return true;
    }
    bool feed_pcm(const int16_t* p, int64_t n) { for (int64_t i = 0; i < n; i += a.stream_piece) if (!part(sd_stream_push(st, p + i, n - i < a.stream_piece ? n - i : a.stream_piece)) || !piece_done()) return false; return true; }
    bool feed_f32(const float* p, int64_t n) { for (int64_t i = 0; i < n; i += a.stream_piece) if (!part(sd_stream_push_f32(st, p + i, n - i < a.stream_piece ? n - i : a.stream_piece)) || !piece_done()) return false; return true; }
};

// the samples sd_diarize_wav would diarize (wav_load: same readers, same --resample / --downmix / --assume-16k rules), pushed in pieces
static bool stream_file(StreamRun& r)
{
    WavLoad f;
    wav_load(r.a.wav, r.a.wav_flags, f);
    if (f.refused()) { fprintf(stderr, "%s\n", f.refusal(r.a.wav).c_str()); return false; }
    if (f.kind == WavLoad::PCM16) return r.feed_pcm(f.pcm, f.n);
    if (f.kind == WavLoad::F32) return r.feed_f32(f.f32, f.n);
    std::vector<float> out;
    const int rc = resample_16k(r.ctx, f, out);
    if (rc != SD_OK) { fprintf(stderr, "resampling failed (%d): %s\n", rc, sd_last_error(r.ctx)); return false; }
    return r.feed_f32(out.data(), (int64_t)out.size());
}

// headerless samples from stdin -- s16le mono at 16 kHz or at --stream-rate HZ, or interleaved frames in the format of --stream-encoding / -channels /
// -channel -- pushed as they arrive: reads of at most 2 MiB, an update block whenever a piece is complete
static bool stream_stdin(StreamRun& r)
{
    const long long piece = r.a.stream_piece;
    const size_t bpf = r.a.stream_fmt ? (size_t)(r.a.stream_enc == SD_ENC_S16 ? 2 : r.a.stream_enc == SD_ENC_F32 ? 4 : 1) * (size_t)r.a.stream_channels : 2;      // bytes of a frame
    const long long most = (long long)((size_t)(2 << 20) / bpf > 0 ? (size_t)(2 << 20) / bpf : 1);
    const long long cap = piece < most ? piece : most;      // frames of one read
    std::vector<unsigned char> buf((size_t)cap * bpf);
    size_t have = 0;                                 // bytes of buf filled
    long long in_piece = 0;                          // frames of the current piece pushed so far
    for (;;) {
        const long long room = piece - in_piece;     // frames the current piece still takes
        const size_t want = (size_t)(room < cap ? room : cap) * bpf;
        const ssize_t got = read(0, (char*)buf.data() + have, want - have);      // (bytes of a partial frame stay in buf for the next read)
        if (got < 0) { if (errno == EINTR) continue; perror("stdin"); return false; }
        have += (size_t)got;
        if (have == want || (got == 0 && have >= bpf)) {
            const long long m = (long long)(have / bpf);
            if (!r.part(r.a.stream_fmt ? sd_stream_push_audio(r.st, buf.data(), m) : sd_stream_push(r.st, (const int16_t*)buf.data(), m))) return false;
            have -= (size_t)m * bpf;                 // (only at the end of the input: a partial frame, which is dropped)
            in_piece += m;
            if (in_piece == piece) { if (!r.piece_done()) return false; in_piece = 0; }
        }
        if (got == 0) {                              // end of input: the last piece is a partial one
            if (have > 0 && r.a.stream_fmt) fprintf(stderr, "stdin: %zu bytes of a partial frame at the end of the input are dropped\n", have);
            return in_piece == 0 || r.piece_done();
        }
    }
}

static int run_stream(const Args& a)
{
    Gallery g;
    if (a.speakers && !g.read(a.speakers)) return 1;
    sd_ctx* ctx = open_context(a);
    if (!ctx) return 1;
    sd_stream* st = nullptr;
    sd_roster* roster = nullptr;
    StreamRun r{ctx, st, a};
    auto leave = [&](int rc) { sd_free_turns(r.turns); sd_stream_close(r.st); sd_roster_close(roster); sd_destroy(ctx); return rc; };      // every way out gives back what it holds
    if (a.enrolled) { if (!enrol_gallery(ctx, a, g)) return leave(1); r.gal = &g; }
    if (sd_stream_open(ctx, &r.st) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return leave(1); }
    if (a.stream_window >= 0 && sd_stream_set_window(r.st, a.stream_window) != SD_OK) { fprintf(stderr, "%s\n", sd_last_error(ctx)); return leave(1); }
    if (a.stream_roster && (sd_roster_open(SD_EMB_DIM, &roster) != SD_OK || sd_stream_set_roster(r.st, roster) != SD_OK)) { fprintf(stderr, "--stream-roster: no roster (%s)\n", sd_last_error(ctx)); return leave(1); }
    if (a.stream_rate > 0 && sd_stream_set_input_rate(r.st, (int32_t)a.stream_rate) != SD_OK) { fprintf(stderr, "--stream-rate %lld: %s\n", a.stream_rate, sd_last_error(ctx)); return leave(1); }
    if (a.stream_fmt && sd_stream_set_input_format(r.st, a.stream_enc, (int32_t)a.stream_channels, (int32_t)a.stream_channel) != SD_OK) { fprintf(stderr, "--stream-encoding / --stream-channels / --stream-channel: %s\n", sd_last_error(ctx)); return leave(1); }
    const bool fed = std::string(a.wav) == "-" ? stream_stdin(r) : stream_file(r);
    if (fed && a.stream_rate > 0) {      // the outputs behind the last final one, before the final turns
        const int rc = sd_stream_end_input(r.st);
        if (rc != SD_OK) { fprintf(stderr, "sd_stream_end_input failed (%d): %s\n", rc, sd_last_error(ctx)); return leave(1); }
        r.bill();
    }
    if (!fed || !r.ask()) return leave(1);
    int64_t n = 0, total = 0;
    sd_stream_info(r.st, &n, nullptr, &total);
    if (total <= 0) { fprintf(stderr, "diarization failed (%d): audio of %lld samples yields no chunk\n", SD_ERR_SHORT, (long long)n); return leave(1); }
    std::vector<const char*> names;
    if (a.speakers && !cluster_names(ctx, a, g, names)) return leave(1);
    print_block(ctx, r.turns, r.nt, a, r.ms, a.speakers ? &names : nullptr);
    return leave(0);
}

static bool read_all(int fd, void* buf, size_t n)
{
    size_t got = 0;
    while (got < n) { const ssize_t r = read(fd, (char*)buf + got, n - got); if (r <= 0) return false; got += (size_t)r; }
    return true;
}

// one rank of the sharded job.  id_rd = pipe this rank reads the rendezvous id from (ranks > 0), id_wr = the pipes rank 0 writes it to;
// ready_wr = pipe on which this rank (> 0) tells rank 0 that its wav and its context are in place, ready_rd = rank 0's ends.
// Rank 0 mints the id only after EVERY rank has reported ready: a rank that cannot start (no such GPU, unreadable wav, bad model)
// ends the job before anyone enters ncclCommInitRank, where a missing peer would mean waiting forever.
static int run_rank(const Args& a, int rank, int world, int id_rd, const std::vector<int>& id_wr, int ready_wr, const std::vector<int>& ready_rd)
{
    int16_t* pcm = nullptr; int64_t n = 0; int32_t sr = 0, ch = 0;
    if (sd_read_wav(a.wav, &pcm, &n, &sr, &ch) != SD_OK) {
        fprintf(stderr, "rank %d: cannot read 16-bit PCM wav: %s (--gpus needs 16-bit samples)\n", rank, a.wav);
        return 1;
    }
    if (sr != 16000 || a.wav_flags) {
        fprintf(stderr, "rank %d: %s: %d Hz%s; --gpus shards a 16 kHz mono 16-bit recording as it is (resample / downmix it first: --resample and --downmix "
                        "are single-GPU options)\n", rank, a.wav, sr, a.wav_flags ? ", --resample / --downmix given" : "");
        return 1;
    }
    sd_ctx* ctx = open_context(a, rank, ("rank " + std::to_string(rank) + ": ").c_str());
    if (!ctx) return 1;
    unsigned char id[SD_COMM_ID_BYTES];
    if (rank == 0) {
        for (size_t q = 0; q < ready_rd.size(); ++q) {
            char ok = 0;
            if (!read_all(ready_rd[q], &ok, 1) || ok != 1) { fprintf(stderr, "rank 0: rank %zu did not come up; no job\n", q + 1); return 1; }
        }
        if (sd_comm_unique_id(id) != SD_OK) { fprintf(stderr, "rank 0: sd_comm_unique_id failed\n"); return 1; }
        for (int fd : id_wr) if (write(fd, id, sizeof(id)) != (ssize_t)sizeof(id)) { fprintf(stderr, "rank 0: cannot hand the rendezvous id over\n"); return 1; }
    } else {
        const char ok = 1;
        if (write(ready_wr, &ok, 1) != 1) { fprintf(stderr, "rank %d: rank 0 is gone\n", rank); return 1; }
        if (!read_all(id_rd, id, sizeof(id))) { fprintf(stderr, "rank %d: no rendezvous id from rank 0\n", rank); return 1; }
    }
    if (sd_comm_init(ctx, id, rank, world) != SD_OK) { fprintf(stderr, "rank %d: sd_comm_init failed: %s\n", rank, sd_last_error(ctx)); return 1; }
    std::vector<int64_t> ranges((size_t)world * 2);
    sd_shard_plan(n, world, -1, ranges.data(), nullptr);
    const int64_t lo = ranges[2 * (size_t)rank], hi = ranges[2 * (size_t)rank + 1];
    int64_t s0 = lo * SD_HOP, s1 = hi > lo ? (hi - 1) * SD_HOP + SD_CHUNK : s0;
    if (s1 > n) s1 = n;
    if (s0 > n) s0 = n;
    sd_turn* turns = nullptr; int64_t nt = 0;
    // collective failure: if any rank fails in its part, every rank gets a non-OK return here (comm.cpp) and exits 1
    const int rc = sd_diarize_sharded(ctx, pcm + s0, s0, s1 - s0, n, &turns, &nt);
    if (rc != SD_OK) { fprintf(stderr, "rank %d: diarization failed (%d): %s\n", rank, rc, sd_last_error(ctx)); return 1; }
    if (rank == 0) print_block(ctx, turns, nt, a);
    sd_free_turns(turns);
    sd_free_pcm(pcm);
    sd_destroy(ctx);
    return 0;
}

int main(int argc, char* argv[])
{
    g_t_main = wall_ms();
    Args a;
    std::vector<const char*> pos;
    for (int i = 1; i < argc; ++i) {
        const std::string s(argv[i]);
        if (s == "--gpus" && i + 1 < argc) a.gpus = atoi(argv[++i]);
        else if (s == "--rttm" && i + 1 < argc) a.rttm = argv[++i];
        else if (s == "--relabel") a.relabel = true;
        else if (s == "--dump-steps" && i + 1 < argc) a.dump_dir = argv[++i];
        else if (s == "--dump-level" && i + 1 < argc) a.dump_level = atoi(argv[++i]);
        else if (s == "--resample") a.wav_flags |= SD_WAV_RESAMPLE;
        else if (s == "--downmix") a.wav_flags |= SD_WAV_DOWNMIX;
        else if (s == "--assume-16k") a.wav_flags |= SD_WAV_ASSUME_16K;
        else if (s == "--precision" && i + 1 < argc) {
            const std::string v(argv[++i]);
            if (v == "f32") a.precision = 0; else if (v == "f16") a.precision = 1; else if (v == "x3") a.precision = 3;
            else { fprintf(stderr, "--precision takes f32, f16 or x3\n"); return 2; }
        }
        else if (s == "--clustering-method" || s == "--clustering-threshold" || s == "--min-cluster-size") {
            // checked here, before any context exists: a bad value never reaches the GPU
            if (i + 1 >= argc) { fprintf(stderr, "usage: %s needs a value\n", s.c_str()); return 2; }
            const char* v = argv[++i];
            char* end = nullptr;
            if (s == "--clustering-method") {
                a.cl_method = sd_linkage_method_from_name(v);
                if (a.cl_method < 0) { fprintf(stderr, "usage: --clustering-method takes single, complete, average, centroid, median, ward or weighted (got '%s')\n", v); return 2; }
            } else if (s == "--clustering-threshold") {
                a.cl_threshold = strtod(v, &end);
                if (end == v || *end || !(a.cl_threshold >= 0.0 && a.cl_threshold <= 2.0)) { fprintf(stderr, "usage: --clustering-threshold takes a number in [0, 2] (got '%s')\n", v); return 2; }
            } else {
                a.cl_min_size = strtoll(v, &end, 10);
                if (end == v || *end || a.cl_min_size < 1 || a.cl_min_size > 0x7fffffff) { fprintf(stderr, "usage: --min-cluster-size takes an integer >= 1 (got '%s')\n", v); return 2; }
            }
        }
        else if (s == "--max-num-embeddings" || s == "--clustering-seed") {
            if (i + 1 >= argc) { fprintf(stderr, "usage: %s needs a value\n", s.c_str()); return 2; }
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            const long long x = strtoll(v, &end, 10);
            const bool number = end != v && !*end && errno != ERANGE;
            if (s == "--max-num-embeddings") {
                if (!number || (x != -1 && x < 1)) { fprintf(stderr, "usage: --max-num-embeddings takes an integer >= 1, or -1 for every row (got '%s')\n", v); return 2; }
                a.cl_max_num = x;
            } else {
                if (!number) { fprintf(stderr, "usage: --clustering-seed takes a 64-bit integer (got '%s')\n", v); return 2; }
                a.cl_seed = x; a.cl_seed_set = true;
            }
        }
        else if (s == "--stream-window") {
            if (i + 1 >= argc) { fprintf(stderr, "usage: --stream-window needs a value\n"); return 2; }
            const char* v = argv[++i];
            char* end = nullptr;
            const double sec = strtod(v, &end);
            if (end == v || *end || !(sec > 0.0) || sec > 1e9) { fprintf(stderr, "usage: --stream-window takes a number of seconds > 0 (got '%s')\n", v); return 2; }
            a.stream_window = (long long)ceil(sec / 16.0);      // blocks of 32 chunks = 256 000 samples
        }
        else if (s == "--many") {
            if (i + 1 >= argc || !argv[i + 1][0]) { fprintf(stderr, "usage: --many needs a list file\n"); return 2; }
            a.many = argv[++i];
        }
        else if (s == "--skip-overlap") a.skip_overlap = true;
        else if (s == "--uem-from-ref") a.uem_from_ref = true;
        else if (s == "--score" || s == "--tune" || s == "--collar" || s == "--thresholds" || s == "--min-cluster-sizes") {
            // checked here: a bad grid is a usage error before any context is created
            if (i + 1 >= argc || !argv[i + 1][0]) { fprintf(stderr, "usage: %s needs a value\n", s.c_str()); return 2; }
            const char* v = argv[++i];
            char* end = nullptr;
            if (s == "--score") a.score = v;
            else if (s == "--tune") a.tune = v;
            else if (s == "--collar") {
                a.collar = strtod(v, &end);
                if (end == v || *end || !(a.collar >= 0.0) || a.collar > 1e300) { fprintf(stderr, "usage: --collar takes a number of seconds >= 0 (got '%s')\n", v); return 2; }
            } else if (s == "--thresholds") {
                const double lo = strtod(v, &end);
                bool ok = end != v && *end == ':';
                const char* p2 = ok ? end + 1 : v;
                const double hi = ok ? strtod(p2, &end) : 0.0;
                ok = ok && end != p2 && *end == ':';
                const char* p3 = ok ? end + 1 : v;
                const long long cnt = ok ? strtoll(p3, &end, 10) : 0;
                ok = ok && end != p3 && !*end && lo >= 0.0 && hi >= lo && hi <= 2.0 && cnt >= 1 && cnt <= 100000;
                if (!ok) { fprintf(stderr, "usage: --thresholds takes LO:HI:N with 0 <= LO <= HI <= 2 and 1 <= N <= 100000 (got '%s')\n", v); return 2; }
                a.thresholds.clear();
                for (long long q = 0; q < cnt; ++q) a.thresholds.push_back(cnt == 1 ? lo : lo + (hi - lo) * (double)q / (double)(cnt - 1));
            } else {
                a.min_sizes.clear();
                for (const char* q = v;;) {
                    const long long m = strtoll(q, &end, 10);
                    if (end == q || (*end && *end != ',') || m < 1 || m > 0x7fffffff) { fprintf(stderr, "usage: --min-cluster-sizes takes integers >= 1 separated by commas (got '%s')\n", v); return 2; }
                    a.min_sizes.push_back(m);
                    if (!*end) break;
                    q = end + 1;
                }
            }
        }
        else if (s == "--stream-updates") a.stream_updates = true;
        else if (s == "--stream-roster") a.stream_roster = true;
        else if (s == "--enrolled") a.enrolled = true;
        else if (s == "--stream") {
            if (i + 1 >= argc) { fprintf(stderr, "usage: --stream needs a value\n"); return 2; }
            const char* v = argv[++i];
            char* end = nullptr;
            const double sec = strtod(v, &end);
            if (end == v || *end || !(sec > 0.0) || !(sec * SD_SAMPLE_RATE >= 1.0) || sec > 86400.0) { fprintf(stderr, "usage: --stream takes a number of seconds > 0, at least one sample and at most a day (got '%s')\n", v); return 2; }
            a.stream_piece = (long long)(sec * SD_SAMPLE_RATE + 0.5);
            a.stream_sec = sec;
        }
        else if (s == "--stream-rate") {
            if (i + 1 >= argc) { fprintf(stderr, "usage: --stream-rate needs a value\n"); return 2; }
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            a.stream_rate = strtoll(v, &end, 10);
            if (end == v || *end || errno || a.stream_rate < 1 || a.stream_rate > 0x7fffffff) { fprintf(stderr, "usage: --stream-rate takes a sample rate in Hz, an integer > 0 (got '%s')\n", v); return 2; }
        }
        else if (s == "--stream-encoding") {
            if (i + 1 >= argc) { fprintf(stderr, "usage: --stream-encoding needs a value\n"); return 2; }
            const std::string v = argv[++i];
            if (v == "s16") a.stream_enc = SD_ENC_S16; else if (v == "f32") a.stream_enc = SD_ENC_F32; else if (v == "mulaw") a.stream_enc = SD_ENC_MULAW; else if (v == "alaw") a.stream_enc = SD_ENC_ALAW;
            else { fprintf(stderr, "usage: --stream-encoding takes s16, f32, mulaw or alaw (got '%s')\n", v.c_str()); return 2; }
            a.stream_fmt = true;
        }
        else if (s == "--stream-channels") {
            if (i + 1 >= argc) { fprintf(stderr, "usage: --stream-channels needs a value\n"); return 2; }
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            a.stream_channels = strtoll(v, &end, 10);
            if (end == v || *end || errno || a.stream_channels < 1 || a.stream_channels > 65535) { fprintf(stderr, "usage: --stream-channels takes a channel count, an integer from 1 to 65535 (got '%s')\n", v); return 2; }
            a.stream_fmt = true;
        }
        else if (s == "--stream-channel") {
            if (i + 1 >= argc) { fprintf(stderr, "usage: --stream-channel needs a value\n"); return 2; }
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            if (std::string(v) == "mean") a.stream_channel = -1;
            else {
                a.stream_channel = strtoll(v, &end, 10);
                if (end == v || *end || errno || a.stream_channel < 0 || a.stream_channel > 65534) { fprintf(stderr, "usage: --stream-channel takes a channel, an integer >= 0, or mean (got '%s')\n", v); return 2; }
            }
            a.stream_fmt = true;
        }
        else if (s == "--speakers" || s == "--speakers-threshold" || s == "--enroll" || s == "--enroll-span") {
            // checked here as well: a usage error before any context is created
            const int need = s == "--enroll-span" ? 2 : 1;
            if (i + need >= argc) { fprintf(stderr, "usage: %s needs %s\n", s.c_str(), need == 2 ? "START END" : "a value"); return 2; }
            const char* v = argv[++i];
            char* end = nullptr;
            if (s == "--speakers") {
                if (!v[0]) { fprintf(stderr, "usage: --speakers takes a file name\n"); return 2; }
                a.speakers = v;
            } else if (s == "--speakers-threshold") {
                a.speakers_threshold = strtod(v, &end);
                if (end == v || *end || !(a.speakers_threshold >= 0.0 && a.speakers_threshold <= 2.0)) { fprintf(stderr, "usage: --speakers-threshold takes a number in [0, 2] (got '%s')\n", v); return 2; }
            } else if (s == "--enroll") {
                bool ok = v[0] != 0;
                for (const char* p = v; *p; ++p) if (*p == '#' || *p == ' ' || (*p >= '\t' && *p <= '\r')) ok = false;
                if (!ok) { fprintf(stderr, "usage: --enroll takes a name without white space or # (got '%s')\n", v); return 2; }
                a.enroll = v;
            } else {
                const char* v2 = argv[++i];
                char* end2 = nullptr;
                const double t0 = strtod(v, &end), t1 = strtod(v2, &end2);
                if (end == v || *end || end2 == v2 || *end2 || !(t0 >= 0.0) || !(t1 >= t0) || t1 > 1e300) { fprintf(stderr, "usage: --enroll-span takes START END in seconds, 0 <= START <= END (got '%s' '%s')\n", v, v2); return 2; }
                a.enroll_spans.push_back(sd_turn{t0, t1, 0, 0});
            }
        }
        else if (s == "--activity-hamming") a.act_hamming = true;
        else if (s == "--activity" || s == "--activity-onset" || s == "--activity-offset" || s == "--activity-min-on" || s == "--activity-min-off") {
            // checked here too: a usage error before any context is created
            if (i + 1 >= argc) { fprintf(stderr, "usage: %s needs a value\n", s.c_str()); return 2; }
            const char* v = argv[++i];
            if (s == "--activity") {
                if (std::string(v) == "speech") a.activity = SD_ACTIVITY_SPEECH; else if (std::string(v) == "overlap") a.activity = SD_ACTIVITY_OVERLAP;
                else { fprintf(stderr, "usage: --activity takes speech or overlap (got '%s')\n", v); return 2; }
            } else {
                const int q = s == "--activity-onset" ? 0 : s == "--activity-offset" ? 1 : s == "--activity-min-on" ? 2 : 3;
                char* end = nullptr;
                a.act[q] = strtod(v, &end);
                if (end == v || *end || !(a.act[q] >= 0.0) || (q < 2 && a.act[q] > 1.0) || a.act[q] > 1e300) {
                    fprintf(stderr, "usage: %s takes %s (got '%s')\n", s.c_str(), q < 2 ? "a number in [0, 1]" : "a number of seconds >= 0", v); return 2;
                }
            }
        }
        else pos.push_back(argv[i]);
    }
    if (a.activity >= 0 && a.gpus > 1) { fprintf(stderr, "usage: --activity runs on one GPU; --gpus %d is refused\n", a.gpus); return 2; }
    if (a.stream_piece > 0 && a.gpus > 1) { fprintf(stderr, "usage: --stream runs on one GPU; --gpus %d is refused\n", a.gpus); return 2; }
    if (a.stream_piece > 0 && a.activity >= 0) { fprintf(stderr, "usage: --stream gives speaker turns; --activity is refused with it\n"); return 2; }
    if (a.stream_piece > 0 && a.dump_dir) { fprintf(stderr, "usage: --dump-steps describes one whole-path inference; --stream is refused with it\n"); return 2; }
    if (a.stream_window >= 0 && a.stream_piece <= 0) { fprintf(stderr, "usage: --stream-window needs --stream SECONDS\n"); return 2; }
    if (a.cl_max_num >= 1 && a.dump_dir) { fprintf(stderr, "usage: --dump-steps describes the reference's flow, which clusters every train row; --max-num-embeddings is refused with it\n"); return 2; }
    if (a.stream_rate > 0 && (a.stream_piece <= 0 || pos.size() < 3 || std::string(pos[2]) != "-")) { fprintf(stderr, "usage: --stream-rate gives the rate of the samples on stdin: it needs --stream SECONDS and - in place of the wav file\n"); return 2; }
    if (a.stream_fmt && (a.stream_piece <= 0 || pos.size() < 3 || std::string(pos[2]) != "-")) { fprintf(stderr, "usage: --stream-encoding, --stream-channels and --stream-channel give the format of the frames on stdin: they need --stream SECONDS and - in place of the wav file\n"); return 2; }
    if (a.stream_fmt && a.stream_channel >= a.stream_channels) { fprintf(stderr, "usage: --stream-channel %lld is outside the %lld channels of --stream-channels\n", a.stream_channel, a.stream_channels); return 2; }
    if (a.stream_rate > 0) { a.stream_piece = (long long)(a.stream_sec * (double)a.stream_rate + 0.5); if (a.stream_piece < 1) a.stream_piece = 1; }      // SECONDS are seconds of audio
    if (a.stream_roster && a.stream_piece <= 0) { fprintf(stderr, "usage: --stream-roster needs --stream SECONDS\n"); return 2; }
    if (a.stream_roster && (a.speakers || a.relabel)) { fprintf(stderr, "usage: --stream-roster prints roster ids; --speakers and --relabel name and renumber raw labels and are refused with it\n"); return 2; }
    if (a.stream_updates && a.stream_piece <= 0) { fprintf(stderr, "usage: --stream-updates needs --stream SECONDS\n"); return 2; }
    if (pos.size() >= 3 && std::string(pos[2]) == "-" && a.stream_piece <= 0) { fprintf(stderr, "usage: samples from stdin (-) need --stream SECONDS\n"); return 2; }
    if (a.enroll && !a.speakers) { fprintf(stderr, "usage: --enroll NAME needs --speakers FILE, the voiceprint file to write\n"); return 2; }
    if (!a.enroll && !a.enroll_spans.empty()) { fprintf(stderr, "usage: --enroll-span needs --enroll NAME\n"); return 2; }
    if (a.speakers_threshold >= 0.0 && (!a.speakers || a.enroll)) { fprintf(stderr, "usage: --speakers-threshold needs --speakers FILE (and no --enroll)\n"); return 2; }
    if (a.speakers && a.activity >= 0) { fprintf(stderr, "usage: --speakers names the clusters of a diarization; --activity is refused with it\n"); return 2; }
    if (a.speakers && a.gpus > 1) { fprintf(stderr, "usage: --speakers runs on one GPU; --gpus %d is refused\n", a.gpus); return 2; }
    if (a.enrolled && !a.speakers) { fprintf(stderr, "usage: --enrolled needs --speakers FILE, the voiceprints to enrol\n"); return 2; }
    if (a.enrolled && a.enroll) { fprintf(stderr, "usage: --enrolled enrols the voiceprints of FILE for a diarization; --enroll runs none and is refused with it\n"); return 2; }
    if (a.enrolled && a.dump_dir) { fprintf(stderr, "usage: --dump-steps describes the reference's flow; --enrolled is refused with it\n"); return 2; }
    if (a.enroll && (a.stream_piece > 0 || a.dump_dir)) { fprintf(stderr, "usage: --enroll runs no diarization; --stream and --dump-steps are refused with it\n"); return 2; }
    if (a.many && (a.gpus > 1 || a.stream_piece > 0 || a.activity >= 0 || a.dump_dir || a.enroll)) { fprintf(stderr, "usage: --many diarizes a list of recordings on one GPU; --gpus N, --stream, --activity, --dump-steps and --enroll are refused with it\n"); return 2; }
    if (a.many && pos.size() != 2) { fprintf(stderr, "usage: --many LIST takes the place of the wav argument\n"); return 2; }
    if (a.score && a.tune) { fprintf(stderr, "usage: --score scores one diarization, --tune a grid of them; give one of the two\n"); return 2; }
    if ((a.score || a.tune) && (a.gpus > 1 || a.stream_piece > 0 || a.activity >= 0 || a.many || a.enroll)) { fprintf(stderr, "usage: %s scores the speaker turns of one file on one GPU; --gpus N, --stream, --activity, --many and --enroll are refused with it\n", a.score ? "--score" : "--tune"); return 2; }
    if (a.tune && (a.enrolled || a.dump_dir)) { fprintf(stderr, "usage: --tune cuts one dendrogram many times; --enrolled and --dump-steps are refused with it\n"); return 2; }
    if (a.tune && a.thresholds.empty()) { fprintf(stderr, "usage: --tune REF.rttm needs --thresholds LO:HI:N\n"); return 2; }
    if (!a.tune && (!a.thresholds.empty() || !a.min_sizes.empty())) { fprintf(stderr, "usage: --thresholds and --min-cluster-sizes need --tune REF.rttm\n"); return 2; }
    if (!a.tune && !a.score && (a.collar > 0.0 || a.skip_overlap || a.uem_from_ref)) { fprintf(stderr, "usage: --collar, --skip-overlap and --uem-from-ref need --score or --tune REF.rttm\n"); return 2; }
    if (a.tune && a.min_sizes.empty()) a.min_sizes.push_back(a.cl_min_size >= 1 ? a.cl_min_size : 0);      // (0 = the context's option)
    if (a.score || a.tune) {
        sd_turn* rt = nullptr; int64_t rn = 0;
        if (sd_read_rttm(a.score ? a.score : a.tune, nullptr, &rt, &rn, nullptr, nullptr) != SD_OK) { fprintf(stderr, "usage: %s REF.rttm: %s\n", a.score ? "--score" : "--tune", sd_score_error()); return 2; }
        a.ref.assign(rt, rt + rn);
        sd_free_turns(rt);
    }
    if (a.many) { a.seg = pos[0]; a.emb = pos[1]; return run_many(a); }
    if (pos.size() < 3) {
        printf("program [segment model file] [embeding model file] [wave file]\n");   // sd.cpp:3423
        return 0;
    }
    a.seg = pos[0]; a.emb = pos[1]; a.wav = pos[2];
    if (a.enroll) return run_enroll(a);
    if (a.tune) return run_tune(a);
    if (a.stream_piece > 0) return run_stream(a);
    if (a.gpus <= 1) return run_single(a);

    // ---- launcher: nothing below touches HIP in this process.  id pipes carry the rendezvous id from rank 0 to rank r,
    // ready pipes one byte from rank r to rank 0.
    const int world = a.gpus;
    std::vector<int> id_rd((size_t)world, -1), id_wr((size_t)world, -1), rdy_rd((size_t)world, -1), rdy_wr((size_t)world, -1);
    for (int r = 1; r < world; ++r) {
        int fd[2];
        if (pipe(fd) != 0) { perror("pipe"); return 1; }
        id_rd[(size_t)r] = fd[0]; id_wr[(size_t)r] = fd[1];
        if (pipe(fd) != 0) { perror("pipe"); return 1; }
        rdy_rd[(size_t)r] = fd[0]; rdy_wr[(size_t)r] = fd[1];
    }
    fflush(stdout); fflush(stderr);
    std::vector<pid_t> kids;
    for (int r = 0; r < world; ++r) {
        const pid_t pid = fork();
        if (pid < 0) { perror("fork"); for (pid_t k : kids) kill(k, SIGKILL); return 1; }
        if (pid == 0) {
            signal(SIGPIPE, SIG_IGN);           // a write to a dead rank's pipe is an error return, not a kill
            // keep only this rank's ends: a rank that dies closes its pipes, so nobody blocks on a read forever
            std::vector<int> my_id_wr, my_rdy_rd;
            for (int q = 1; q < world; ++q) {
                if (r == 0) { close(id_rd[(size_t)q]); close(rdy_wr[(size_t)q]); my_id_wr.push_back(id_wr[(size_t)q]); my_rdy_rd.push_back(rdy_rd[(size_t)q]); }
                else { close(id_wr[(size_t)q]); close(rdy_rd[(size_t)q]); if (q != r) { close(id_rd[(size_t)q]); close(rdy_wr[(size_t)q]); } }
            }
            const int rc = run_rank(a, r, world, r > 0 ? id_rd[(size_t)r] : -1, my_id_wr, r > 0 ? rdy_wr[(size_t)r] : -1, my_rdy_rd);
            fflush(stdout); fflush(stderr);
            _exit(rc);
        }
        kids.push_back(pid);
    }
    for (int r = 1; r < world; ++r) { close(id_rd[(size_t)r]); close(id_wr[(size_t)r]); close(rdy_rd[(size_t)r]); close(rdy_wr[(size_t)r]); }
    // reap in completion order; the first rank that ends badly ends the job: the others (which may be waiting for it inside RCCL)
    // are killed by their exact pids and reaped
    int worst = 0;
    size_t left = kids.size();
    while (left > 0) {
        int st = 0;
        const pid_t pid = waitpid(-1, &st, 0);
        if (pid < 0) { worst = 1; break; }
        size_t which = kids.size();
        for (size_t i = 0; i < kids.size(); ++i) if (kids[i] == pid) which = i;
        if (which == kids.size()) continue;
        kids[which] = -1; --left;
        if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) {
            worst = 1;
            fprintf(stderr, "launcher: rank %zu ended with %s %d; stopping the other ranks\n", which, WIFEXITED(st) ? "exit code" : "signal", WIFEXITED(st) ? WEXITSTATUS(st) : WTERMSIG(st));
            // a rank whose own failure is collective (comm.cpp) exits by itself within moments: give the others a short grace period
            // so that their reasons reach stderr, then kill what is left
            for (int spin = 0; spin < 100 && left > 0; ++spin) {
                int st2 = 0;
                const pid_t p2 = waitpid(-1, &st2, WNOHANG);
                if (p2 > 0) { for (size_t i = 0; i < kids.size(); ++i) if (kids[i] == p2) { kids[i] = -1; --left; } }
                else usleep(20000);
            }
            for (size_t i = 0; i < kids.size(); ++i) if (kids[i] > 0) kill(kids[i], SIGKILL);
            for (size_t i = 0; i < kids.size(); ++i) if (kids[i] > 0) { int st3 = 0; (void)waitpid(kids[i], &st3, 0); kids[i] = -1; }
            left = 0;
        }
    }
    return worst;
}
