/*
 * wseg.h — C-ABI of libwseg.so, the MI355X (gfx950) hot path of whisperseg_amd.
 *
 * The reference (nianlonggu/WhisperSeg) has no FFI of its own: its boundary is Python duck-typing
 * inside model.py.  Each entry point below therefore cites the reference call (file:line, relative to
 * the reference repo root) whose device work it replaces; the Python host side in
 * whisperseg_amd/{audio_utils,model,engine}.py binds these with ctypes and mirrors the reference's
 * class/method surface.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  Every pointer documented "device" is a HIP device
 *     pointer owned by the caller (PyTorch-ROCm allocates; the library never allocates or frees device
 *     memory and never takes ownership).  `stream` is a hipStream_t passed as void* (NULL = default).
 *   - Every function returns 0 on success, a negative wseg_status otherwise; wseg_last_error()
 *     returns a thread-local message for the last failure.
 *   - Functions are thread-compatible: distinct models / distinct streams may be used concurrently
 *     from distinct host threads (the reference calls its backend from one Python thread per device,
 *     model.py:173-184).
 */
#ifndef WSEG_H
#define WSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WSEG_ABI_VERSION 5

typedef enum {
  WSEG_OK = 0,
  WSEG_ERR_INVALID = -1,    /* bad argument / unsupported geometry */
  WSEG_ERR_HIP = -2,        /* a HIP runtime call or kernel launch failed */
  WSEG_ERR_STATE = -3,      /* model not fully populated, workspace too small, ... */
  WSEG_ERR_NO_DEVICE = -4   /* no gfx950 device visible */
} wseg_status;

typedef enum {
  WSEG_F32 = 0,             /* exact-parity mode: fp32 storage; GEMMs on the fp32 matrix cores (v_mfma_f32_32x32x2_f32 / 16x16x4_f32 are
                             * k-ordered fmaf chains bit for bit: tested identical to the VALU kernels they replaced) */
  WSEG_BF16 = 1,            /* bfloat16 storage + MFMA, fp32 accumulation */
  WSEG_F16 = 2,             /* IEEE half storage + MFMA, fp32 accumulation (reference WhisperSegmenterFast: CT2 float16, model.py:691) */
  /* Split-precision modes (the reference's own arithmetic is fp32 everywhere, model.py:655-666): fp32 storage and fp32
   * arithmetic for everything but the GEMMs; GEMM operands (activations and weights) are carried as hi + lo 16-bit pairs
   * and multiplied as hi*hi + hi*lo + lo*hi on the 16-bit matrix cores with fp32 accumulation (3 MFMAs per product,
   * ~2^-16 (bf16) / ~2^-21 (half) relative operand error instead of 2^-8 / 2^-11).  Weight matrices ("*.w", "dec.tok")
   * are attached pre-split: rows of 2K 16-bit words, every 32 logical columns as [32 hi | 32 lo]
   * (whisperseg_amd/engine.py::split_operand); every other tensor is float32. */
  WSEG_BF16X3 = 3,
  WSEG_F16X3 = 4,
  /* Mixed split-precision mode: WSEG_F16X3 everywhere outside the GEMMs; a GEMM takes hi*hi on the IEEE-half matrix cores and the
   * two cross terms hi*lo + lo*hi on the block-scaled MX matrix cores (fp6 e2m3 operands with per-32-element e8m0 scales, 4x the
   * 16-bit rate): 3.25 instead of 6 matrix-core issue units per 64 logical columns at a ~2^-15 operand error.  Weight
   * matrices are attached as "M6 rows" produced by wseg_convert_operand from the WSEG_F16X3 rows.  PARITY (r06): rows
   * identical to the reference's on the 200 recordings the mode was designed on, OUTSIDE the north-star tolerance on 10 of 6 000
   * held-out recordings — a fast mode; the Python layer defaults to WSEG_F16X3 (all 6 200 sweep recordings identical, like WSEG_F32). */
  WSEG_F16M6 = 5
} wseg_dtype;

int wseg_abi_version(void);
const char* wseg_last_error(void);
/* Name / gcnArch of the current device, or an error if none is visible. */
int wseg_device_info(char* name_out, size_t name_cap, int* cu_count_out);

/* ------------------------------------------------------------------------------------------------
 * Log-mel front-end.
 * Replaces, per window: reference audio_utils.py:45-76 (WhisperSegFeatureExtractor) ->
 * HF feature_extraction_whisper.py:105-133 (_np_extract_fbank_features) -> HF audio_utils.py:809-1017
 * (spectrogram), and the window slicing / zero padding / column truncation / min-fill of
 * reference model.py:140-161 — all windows of a recording in one launch pair.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_fft;            /* 512 | 1024 | 2048 | 4096 | 8192  (reference audio_utils.py:32-43) */
  int32_t hop;              /* int(spec_time_step * sr)          (reference audio_utils.py:48)    */
  int32_t n_mels;           /* 80 */
  int32_t n_cols;           /* total_spec_columns, 256 .. 3000 (default 1000; reference model.py:153) */
  const float* window;      /* device [n_fft]      periodic Hann                                   */
  const float* twiddle;     /* device [n_fft/2][2] (cos, -sin)(2*pi*k/n_fft)                        */
  const int32_t* mel_start; /* device [n_mels]     first non-zero FFT bin of each filter           */
  const int32_t* mel_count; /* device [n_mels]     number of consecutive non-zero bins             */
  const int32_t* mel_offset;/* device [n_mels]     offset of the filter's weights in mel_weight    */
  const float* mel_weight;  /* device [sum(mel_count)] slaney triangle weights                     */
} wseg_logmel_desc;

/* Bytes of float scratch needed by wseg_logmel_f32 for n_windows windows of win_len samples. */
size_t wseg_logmel_scratch_bytes(const wseg_logmel_desc* d, int32_t n_windows, int64_t win_len);

/*
 * audio      device float32 [n_audio]   the whole recording (mono), resident in HBM
 * win_start  device int64   [n_windows] first sample of each window relative to audio[0]; may be
 *                                        negative (multi-trial left padding, reference model.py:138-143)
 *                                        or run past the end (zero-filled, reference model.py:150)
 * win_len    samples per window = int(total_spec_columns * spec_time_step * sr)  (model.py:133)
 * out        device float32 [n_windows][n_mels][n_cols]
 */
int wseg_logmel_f32(const wseg_logmel_desc* d, const float* audio, int64_t n_audio,
                    const int64_t* win_start, int32_t n_windows, int64_t win_len,
                    void* scratch, size_t scratch_bytes, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rational polyphase resampler (audio ingest).
 * Replaces the resampling half of `librosa.load(path, sr=target)` at reference scripts/segment.py:48,61 and
 * evaluate.py:58.  y[m] = sum_k taps[(m + pre_remove) * down - pre_pad - k * up] * x[k], all device pointers.
 * The Kaiser-windowed-sinc taps and the two alignment integers are produced by whisperseg_amd/resample.py.
 * ---------------------------------------------------------------------------------------------- */
int wseg_resample_f32(const float* x, int64_t n_in, const float* taps, int32_t n_taps, int32_t up, int32_t down,
                      int32_t pre_pad, int32_t pre_remove, float* y, int64_t n_out, void* stream);
/* The same for n_planes signals at once (the channels of a recording kept apart): y[p * y_plane_stride + m] has the bits of
 * wseg_resample_f32's y[m] for the signal x + p * x_plane_stride, 0 <= p < n_planes — the same fmaf chain over the same k, in
 * one launch whatever the number of planes.  Strides in floats, x_plane_stride >= n_in and y_plane_stride >= n_out (both
 * ignored when n_planes == 1); pointers and strides of any float alignment.  n_planes 1..64.
 * taps: wseg_resample_f32's array, as it is (a workgroup lays it out phase-major in LDS itself when it fits there).
 * n_out == 0 launches nothing; n_in == 0 launches no kernel and zero-fills y.  Writes nothing outside the n_planes * n_out
 * addressed floats.  Stream-ordered.  Added without moving WSEG_ABI_VERSION (an addition). */
int wseg_resample_planar_f32(const float* x, int64_t n_in, int64_t x_plane_stride, int32_t n_planes,
                             const float* taps, int32_t n_taps, int32_t up, int32_t down,
                             int32_t pre_pad, int32_t pre_remove,
                             float* y, int64_t n_out, int64_t y_plane_stride, void* stream);
/* A RANGE of the outputs of wseg_resample_planar_f32 from a SEGMENT of each plane: what resamples a recording piece by piece, each
 * piece as soon as it is decoded, with the last frames of the piece before carried over (whisperseg_amd/resample.py stream_plan).
 * x[p * x_plane_stride + (k - x_first)] is input sample k of plane p of the recording, x_first <= k < x_first + x_frames; n_in is the
 * recording's frame count and enters only as the clamp of a chain's last input.  y is the base of plane 0 of the WHOLE output:
 * y[p * y_plane_stride + m] is written for m_first <= m < m_first + m_count and nothing else, with the bits the whole-recording call
 * gives that output (the same fmaf chain over the same inputs; an empty chain gives 0).  wseg_resample_planar_f32 is this call with
 * x_first = 0, x_frames = n_in, m_first = 0, m_count = n_out.
 * Validated before any launch, WSEG_ERR_INVALID with the offending range in wseg_last_error(): every chain of the range must lie
 * inside the segment — first input of output m_first >= x_first, last input of output m_first + m_count - 1 < x_first + x_frames —
 * and 0 <= m_first, m_count >= 0, x_first >= 0, x_frames >= 0, x_first + x_frames <= n_in, x_plane_stride >= x_frames and
 * y_plane_stride >= m_first + m_count (both ignored when n_planes == 1), n_planes 1..64.  Pointers and strides of any float
 * alignment; no 16-byte load crosses an end of the segment.  m_count == 0 launches nothing.  Stream-ordered.
 * Added without moving WSEG_ABI_VERSION (an addition). */
int wseg_resample_planar_range_f32(const float* x, int64_t x_first, int64_t x_frames, int64_t x_plane_stride, int32_t n_planes,
                                   int64_t n_in, const float* taps, int32_t n_taps, int32_t up, int32_t down,
                                   int32_t pre_pad, int32_t pre_remove,
                                   float* y, int64_t m_first, int64_t m_count, int64_t y_plane_stride, void* stream);
/* The launch plan of wseg_resample_planar_f32, which launches from the same function (host arithmetic, no device; n_in, n_out
 * and the two alignment integers are validated only — the plan follows from up, down and n_taps).  *tile: outputs a workgroup
 * takes at a time, a multiple of 64; *x_staged: whether a tile's input window — k_lo of its first output to k_hi of its last —
 * is staged in LDS, and then *window: the floats reserved for it, ceil((tile - 1) * down / up) + ceil(n_taps / up) + 2
 * (0 when the window is read from global memory); *taps_staged: whether the taps are copied to LDS, phase-major.
 * Added without moving WSEG_ABI_VERSION (an addition). */
int wseg_debug_resample_plan(int64_t n_in, int64_t n_out, int32_t n_taps, int32_t up, int32_t down,
                             int32_t pre_pad, int32_t pre_remove,
                             int32_t* tile, int32_t* window, int32_t* x_staged, int32_t* taps_staged);

/* ------------------------------------------------------------------------------------------------
 * Audio sample decode (audio ingest).
 * Replaces the decoding half of `librosa.load(path, sr=None)` at reference scripts/segment.py:48,61 and evaluate.py:58:
 * sample formats widened to float32 in [-1, 1) and channels averaged to mono, with the float32 bits
 * whisperseg_amd/wavio.py::load_wav produces on the host (u8 (x - 128) / 128, s16 x / 2^15, s24 sign-extended / 2^23,
 * s32 one int -> float32 rounding then the exact scale 2^-31, f32 copied, f64 one round-to-nearest-even conversion; channels:
 * numpy's float32 mean(axis=1), i.e. a sum from +0 in numpy's order — left to right below 8 channels, pairwise from 8 on — and
 * one division by float(channels)).  Added without moving WSEG_ABI_VERSION (an addition, see wseg_debug_step_snapshot_*).
 * ---------------------------------------------------------------------------------------------- */
typedef enum { WSEG_PCM_U8 = 0, WSEG_PCM_S16 = 1, WSEG_PCM_S24 = 2, WSEG_PCM_S32 = 3,
               WSEG_PCM_F32 = 4, WSEG_PCM_F64 = 5 } wseg_pcm_format;
/* raw: device, interleaved little-endian frames exactly as they sit in a WAVE data chunk, 16-byte aligned, readable up to
 * the next multiple of 16 bytes behind n_frames * channels * bytes_per_sample.  out: device float32 [n_frames], mono (any
 * float alignment; 16-byte aligned for 16-byte stores).  channels 1..64.  n_frames == 0 launches nothing.  Stream-ordered. */
int wseg_pcm_to_mono_f32(const void* raw, int64_t n_frames, int32_t channels, int32_t format, float* out, void* stream);
/* The channels of a multi-channel recording kept apart (the reference's `librosa.load(..., mono=False)` and `audio[channel_id]`:
 * segment_service.py:73-80, scripts/backend.py:279-282, demo.py:76-78), what wavio.load_wav(mono=False) gives on the host.
 * out[(c - first_channel) * plane_stride + f] = float32 sample of channel c in frame f, for
 * first_channel <= c < first_channel + n_out_channels and 0 <= f < n_frames; same per-sample conversions as
 * wseg_pcm_to_mono_f32, no averaging.  raw: as for wseg_pcm_to_mono_f32 (16-byte aligned, readable to the next
 * multiple of 16 bytes).  out: any float alignment; plane_stride in floats, >= n_frames (ignored when
 * n_out_channels == 1).  Writes nothing outside the n_out_channels * n_frames addressed floats.
 * channels 1..64.  n_frames == 0 launches nothing.  Stream-ordered.  Added without moving WSEG_ABI_VERSION (an addition). */
int wseg_pcm_to_planar_f32(const void* raw, int64_t n_frames, int32_t channels, int32_t format,
                           int32_t first_channel, int32_t n_out_channels,
                           float* out, int64_t plane_stride, void* stream);
/* The same two decodes for every sample encoding the containers of whisperseg_amd/wavio.py carry (WAVE / RF64 / BW64, AIFF /
 * AIFF-C, AU): what wavio.load_audio does on the host, with its float32 bits.  Codes 0..5 are wseg_pcm_format, same numbers, same
 * arithmetic; the big-endian encodings are byte-swapped in registers and then widened as their little-endian siblings; G.711 codes
 * are expanded to int16 with integer arithmetic (the standard's expansion, the tables of libsndfile and CPython's audioop:
 * u-law extremes +-32124, A-law +-32256) and divided by 2^15.  Equality with libsndfile's floats is by construction (integer /
 * 2^(bits-1), G.711 through int16), not pinned by a test.
 * Every other part of the contract is that of wseg_pcm_to_mono_f32 / wseg_pcm_to_planar_f32: raw 16-byte aligned and readable to
 * the next multiple of 16 bytes, out of any float alignment, channels 1..64, numpy's mean over the channels, nothing written
 * outside the addressed floats, n_frames == 0 launches nothing, stream-ordered.  An encoding outside 0..13 is WSEG_ERR_INVALID
 * ("encoding" in wseg_last_error()).  The wseg_pcm_* entry points are these with codes 0..5 and go on rejecting every other code.
 * Added without moving WSEG_ABI_VERSION (an addition). */
typedef enum {                      /* 0..5 are wseg_pcm_format, same numbers, same arithmetic */
  WSEG_ENC_S8 = 6,                  /* signed 8-bit: x / 128 */
  WSEG_ENC_S16BE = 7, WSEG_ENC_S24BE = 8, WSEG_ENC_S32BE = 9,   /* byte-swapped, then as S16 / S24 / S32 */
  WSEG_ENC_F32BE = 10, WSEG_ENC_F64BE = 11,                     /* byte-swapped, then as F32 / F64 */
  WSEG_ENC_ULAW = 12, WSEG_ENC_ALAW = 13   /* G.711: 8 bits -> int16 by the standard expansion, then x / 2^15 */
} wseg_sample_encoding;
int wseg_samples_to_mono_f32(const void* raw, int64_t n_frames, int32_t channels, int32_t encoding, float* out, void* stream);
int wseg_samples_to_planar_f32(const void* raw, int64_t n_frames, int32_t channels, int32_t encoding,
                               int32_t first_channel, int32_t n_out_channels,
                               float* out, int64_t plane_stride, void* stream);
/* The same two decodes for the one BLOCK codec of the ingest, IMA / DVI ADPCM as WAVE carries it (format tag 0x0011, 4 bits per
 * sample; whisperseg_amd/wavio.py::decode_ima_adpcm is the host definition, code 14 = wavio.ENC_IMA_ADPCM on the Python side only:
 * wseg_samples_to_* go on rejecting it, a block file has no frame size).  raw holds n_blocks blocks of block_bytes bytes:
 *   per channel, in channel order, a 4-byte header: int16 LE predictor | u8 step index | u8 reserved; the predictor is also the
 *     block's first sample of that channel;
 *   then groups of 4 bytes per channel, interleaved by channel (8 samples of channel 0, 8 of channel 1, ...), low nibble first.
 * So block_bytes = 4 * channels * (1 + k), k >= 1, at most 65532 bytes per channel, and a block holds spb = 8 k + 1 frames.  Per nibble d, the
 * standard's integer arithmetic: diff = step >> 3 (+ step if d & 4) (+ step >> 1 if d & 2) (+ step >> 2 if d & 1) with step =
 * table[index]; predictor -= diff if d & 8 else += diff, clamped to int16; index += {-1,-1,-1,-1,2,4,6,8}[d & 7], clamped to 0..88
 * (a header index above 88 is taken as 88).  A sample is predictor / 2^15 as for S16, the mono mix numpy's float32 mean as above.
 * n_frames cuts the last block: (n_blocks - 1) * spb < n_frames <= n_blocks * spb (0 for no blocks).  mono: out[f], 0 <= f <
 * n_frames; planar: out[(c - first_channel) * plane_stride + f] for first_channel <= c < first_channel + n_out_channels — only
 * those channels' chains run.  raw: device, 16-byte aligned, readable to the next multiple of 16 bytes behind n_blocks *
 * block_bytes; out of any float alignment; plane_stride in floats, >= n_frames (ignored when n_out_channels == 1); nothing is
 * written outside the addressed floats; channels 1..64; n_blocks == 0 launches nothing; stream-ordered.  Every argument is
 * validated on the host before a launch: WSEG_ERR_INVALID with the argument's name (raw, out, channels, block_bytes, n_blocks,
 * n_frames, first_channel, n_out_channels, plane_stride) in wseg_last_error().
 * Added without moving WSEG_ABI_VERSION (an addition). */
int wseg_ima_adpcm_to_mono_f32(const void* raw, int64_t n_blocks, int32_t block_bytes, int32_t channels,
                               int64_t n_frames, float* out, void* stream);
int wseg_ima_adpcm_to_planar_f32(const void* raw, int64_t n_blocks, int32_t block_bytes, int32_t channels,
                                 int64_t n_frames, int32_t first_channel, int32_t n_out_channels,
                                 float* out, int64_t plane_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-segment acoustic measurements from the resident PCM: the table a segmenter's users compute next (level, peak frequency,
 * centroid, bandwidth per detected call), taken on the device from the float32 samples the front-end saw.
 * whisperseg_amd/measure.py::measure_host is the definition (numpy, float64); the FFT here is fp32, every sum fp64 in a fixed order:
 * the same input gives the same bits on every run and for every grid size.
 * bounds_host: HOST int64 [n_seg][2], the sample range [s0, s1) of every segment, 0 <= s0 <= s1 <= n (overlaps allowed; all time
 * arithmetic is the caller's).  pcm: device float32 [n]; only samples of [s0, s1) are ever read.  n_fft 512 | 1024 | 2048 | 4096 |
 * 8192; frames of n_fft samples start at s0 and lie n_fft / 4 apart, zero-filled from s1 on: one frame up to n_fft samples, else
 * 1 + ceil((s1 - s0 - n_fft) / hop).  window, twiddle: the log-mel descriptor's tables for that n_fft (device [n_fft] periodic
 * Hann, device [n_fft / 2][2] (cos, -sin)(2 pi k / n_fft)).  The band is the bins k_lo .. k_hi, 1 <= k_lo <= k_hi <= n_fft / 2.
 * out: device float32 [n_seg][8], a row per segment, RATE-FREE (no sampling rate enters the call):
 *   0 max |x|   1 sqrt(mean x^2)   2 sign changes between neighbours inside the range, a count   3 lowest bin of the band's maximum
 *   4 centroid, 5 / 6 the 5 % / 95 % points of the band's cumulated power interpolated inside the crossing bin, in bins
 *   7 entropy of the band's normalised power / ln(bins of the band)
 * s1 == s0: eight NaN; a band without power: NaN in 3..7.  Nothing outside the n_seg rows is written.
 * scratch: device, 8-byte aligned, wseg_measure_scratch_bytes(bounds_host, n_seg, n_fft) bytes — host arithmetic, no device; it
 * returns 0 with the reason in wseg_last_error() for invalid bounds (it knows no n: s1 up to 2^52), n_seg < 0 or another n_fft.
 * The call copies what the kernels need of the bounds through a pinned buffer of the library's on the stream and waits for
 * nothing: bounds_host may be reused on return.  n_seg == 0 returns 0 without a launch.  Every argument is validated on the host
 * before a launch (WSEG_ERR_INVALID, the argument's name in wseg_last_error()).  Stream-ordered.
 * $WSEG_MEASURE_GRID: a TEST knob, the cap on the first kernel's grid (the same bits for every value).
 * Added without moving WSEG_ABI_VERSION (an addition).
 * ---------------------------------------------------------------------------------------------- */
size_t wseg_measure_scratch_bytes(const int64_t* bounds_host, int32_t n_seg, int32_t n_fft);
int wseg_measure_segments_f32(const float* pcm, int64_t n, const int64_t* bounds_host, int32_t n_seg,
                              int32_t n_fft, int32_t k_lo, int32_t k_hi, const float* window, const float* twiddle,
                              void* scratch, size_t scratch_bytes, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-segment log-mel patches from the resident PCM: one fixed-size picture per detected call (clustering, embedding, thumbnails),
 * time-normalised — `width` frames per segment at the segment's own spacing.  whisperseg_amd/patches.py::patches_host is the
 * definition (numpy, float64): column c of the segment [s0, s1), L = s1 - s0, is the frame of n_fft samples centred on
 * s0 + ((2c + 1) L) / (2 width) (integers), every index outside [0, n) read as zero (no reflection; the frame does see the
 * recording outside the segment); periodic Hann -> |rfft|^2 -> the descriptor's mel bank -> log10(max(1e-10, .)) ->
 * (max(v, V - 8) + 4) / 4 with V the picture's maximum.  FFT and mel projection are fp32 in a fixed order: the same bits on every
 * run, for every grid size, and for a segment whatever other segments share the call.
 * d: the log-mel descriptor (hop and n_cols are not read; n_fft 512 .. 8192, n_mels 1 .. 96).  bounds_host: HOST int64 [n_seg][2],
 * 0 <= s0 <= s1 <= n (overlaps allowed; all time arithmetic is the caller's).  pcm: device float32 [n], may be null only when
 * n == 0; no sample outside [0, n) is read.  width 1 .. 256.  out: device float32 [n_seg][n_mels][width]; nothing outside it is
 * written.  scratch: device, 8-byte aligned, wseg_patches_scratch_bytes(n_seg, n_mels, width) bytes — host arithmetic, no device;
 * 0 with the reason in wseg_last_error() for n_seg < 0 or n_mels / width out of range.
 * The call copies the bounds through a pinned buffer of the library's on the stream and waits for nothing: bounds_host may be
 * reused on return.  n_seg == 0 returns 0 without a launch.  Every argument is validated on the host before a launch
 * (WSEG_ERR_INVALID, the argument's name in wseg_last_error()).  Stream-ordered.
 * $WSEG_PATCH_GRID: a TEST knob, the cap on both kernels' grids (the same bits for every value).
 * Added without moving WSEG_ABI_VERSION (an addition).
 * ---------------------------------------------------------------------------------------------- */
size_t wseg_patches_scratch_bytes(int32_t n_seg, int32_t n_mels, int32_t width);
int wseg_patches_f32(const wseg_logmel_desc* d, const float* pcm, int64_t n, const int64_t* bounds_host, int32_t n_seg,
                     int32_t width, void* scratch, size_t scratch_bytes, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * k nearest neighbours of every query row among the corpus rows (the graph clustering, embedding and "calls like this one" start
 * from; over the patches above or any float32 rows) under the squared Euclidean distance.  whisperseg_amd/neighbors.py::
 * neighbors_host is the definition (numpy, float64): d(i, j) = sum_c (q[i][c] - x[j][c])^2 in the direct form; the neighbours of
 * row i are the k candidates that come first in the total order (d(i, j), j), ascending.  The m x n matrix never exists: a
 * selection kernel forms |q|^2 + |x|^2 - 2 q.x tile by tile on the fp32 matrix cores (every term one c-ordered fmaf chain: the
 * same bits for every tiling, grid and split) and keeps the k + 8 best per row; a finish kernel recomputes the direct form of
 * those with fp64 accumulation, orders them by (that distance as float32, j) and writes the first k — the selection's
 * cancellation error (<= 2 (d + 4) 2^-24 (|q|^2 + |x|^2)) only matters at the k-th boundary and shows in no reported distance.
 * queries: device float32 [m][d]; corpus: device float32 [n][d] (may be queries); m, n 0 .. 2^31 - 1, d 1 .. 20480, k 1 .. 64.
 * exclude_same_index 1: j == i is no candidate (queries == corpus; by index, not by value).  Inputs must be finite; with
 * non-finite input the order is unspecified, and still nothing outside the outputs and scratch is written, nothing outside
 * queries and corpus read.  index_out: device int32 [m][k]; distance_out: device float32 [m][k]; where a row has fewer than k
 * candidates its tail is -1 / +inf.  scratch: device, 8-byte aligned, wseg_knn_scratch_bytes(m, n, d, k) bytes — host arithmetic,
 * no device, monotone in every argument; 0 with the reason in wseg_last_error() for sizes out of range.
 * m == 0 returns 0 without a launch; n == 0 only fills -1 / +inf.  Every argument is validated on the host before a launch
 * (WSEG_ERR_INVALID, the argument's name in wseg_last_error()).  Stream-ordered, no host synchronisation.
 * $WSEG_KNN_GRID: a TEST knob, the cap on the grids and with it the candidate splits (the same bits for every value).
 * Added without moving WSEG_ABI_VERSION (an addition).
 * ---------------------------------------------------------------------------------------------- */
size_t wseg_knn_scratch_bytes(int64_t m, int64_t n, int32_t d, int32_t k);
int wseg_knn_f32(const float* queries, int64_t m, const float* corpus, int64_t n, int32_t d, int32_t k,
                 int32_t exclude_same_index, void* scratch, size_t scratch_bytes, int32_t* index_out, float* distance_out,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * One Boruvka round of the minimum spanning tree of the rows under the mutual-reachability distance — the N^2 D part of
 * density-based clustering (HDBSCAN, DBSCAN*, robust single linkage) of the patches above or any float32 rows.
 * whisperseg_amd/linkage.py::mst_host is the definition of the tree (numpy, float64) and linkage.py::mst drives the rounds:
 * d32(i, j) = float32(sum_c (x[i][c] - x[j][c])^2) in the direct form, w(i, j) = max(core[i], core[j], d32(i, j)).
 * For every row i the call writes index_out[i] = the j with component[j] != component[i] that comes first in the order
 * (w(i, j), j) and weight_out[i] = w(i, j); -1 / +inf where no such j exists.  The n x n matrix never exists: a selection kernel
 * forms max(core_i, core_j, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) tile by tile on the fp32 matrix cores (every term one c-ordered fmaf
 * chain: the same bits for every tiling, grid and split) and keeps the 1 + 8 best per row; a finish kernel recomputes the direct
 * form of those with fp64 accumulation (symmetric: d32(i, j) and d32(j, i) have the same bits) and writes the first under
 * (exact w, j) — the selection's cancellation error (<= 2 (d + 4) 2^-24 (|x_i|^2 + |x_j|^2)) decides only which nine candidates
 * are looked at and shows in no reported weight.
 * rows: device float32 [n][d]; n 0 .. 2^31 - 1, d 1 .. 20480.  core: device float32 [n], finite, >= 0 (the caller's: for HDBSCAN
 * the squared distance to the s-th nearest other row, wseg_knn_f32's column s - 1).  component: device int32 [n], any values,
 * only compared for equality (a row is of its own component: it is never its own candidate).  Inputs must be finite; with
 * non-finite input the choice is unspecified, and still nothing outside the outputs and scratch is written, nothing outside rows,
 * core and component read.  index_out: device int32 [n]; weight_out: device float32 [n].  scratch: device, 8-byte aligned,
 * wseg_mst_scratch_bytes(n, d) bytes — host arithmetic, no device, monotone in n and d; 0 with the reason in wseg_last_error()
 * for sizes out of range.
 * n == 0 returns 0 without a launch.  Every argument is validated on the host before a launch (WSEG_ERR_INVALID, the argument's
 * name in wseg_last_error()).  Stream-ordered, no host synchronisation.
 * $WSEG_MST_GRID: a TEST knob, the cap on the grids and with it the candidate splits (the same bits for every value).
 * Added without moving WSEG_ABI_VERSION (an addition).
 * ---------------------------------------------------------------------------------------------- */
size_t wseg_mst_scratch_bytes(int64_t n, int32_t d);
int wseg_mst_round_f32(const float* rows, int64_t n, int32_t d, const float* core, const int32_t* component, void* scratch,
                       size_t scratch_bytes, int32_t* index_out, float* weight_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Layout epochs of the 2-D / 3-D embedding of the calls: a synchronous variant of UMAP's optimiser over a weighted graph in CSR
 * form.  whisperseg_amd/embed.py::layout_host is the definition (numpy, float64: the schedule, the counter-based negative samples,
 * a term and the order of an epoch's sums) and embed.py::layout the caller.  The call runs the epochs t0 .. t1 - 1 of total_epochs,
 * one launch each: epoch t gives every vertex i  y[i] + lr (1 - t / total_epochs) G_i, G_i the sum IN CSR ORDER over the entries e
 * of row i that are active in epoch t (((t + 1) rate[e]) >> 16 != (t rate[e]) >> 16) of the attraction term towards indices[e] and
 * then the repulsion terms of n_neg negative samples, all read from the positions epoch t - 1 left — the epochs ping-pong between
 * y_out and scratch and the last one writes y_out.  float64 throughout; with b == 1 (the instance without pow) the positions are
 * the definition's bit for bit, with another b they differ by the two pow functions' difference.
 * indptr: device int64 [n + 1]; indices: device int32 [nnz]; rate: device uint32 [nnz] (0 .. 65536); n 0 .. 2^31 - 1, nnz 0 .. 2^38,
 * dim 2 or 3.  An entry whose index is outside 0 .. n - 1 and the part of a row outside 0 .. nnz contribute nothing, so nothing
 * outside the inputs is read whatever they hold.  y_in, y_out: device float64 [n][dim]; scratch: device, 8-byte aligned,
 * wseg_embed_scratch_bytes(n, dim) bytes — host arithmetic, no device; 0 with the reason in wseg_last_error() for sizes out of
 * range; the three must not overlap.  0 <= t0 < t1 <= total_epochs <= 2^31 - 1; n_neg 0 .. 16; lr, gamma finite, a >= 0, b > 0.
 * n == 0 returns 0 without a launch.  Every argument is validated on the host before a launch (WSEG_ERR_INVALID, the argument's
 * name in wseg_last_error()).  Stream-ordered, no host synchronisation.
 * Added without moving WSEG_ABI_VERSION (an addition).
 * ---------------------------------------------------------------------------------------------- */
size_t wseg_embed_scratch_bytes(int64_t n, int32_t dim);
int wseg_embed_epochs_f64(const int64_t* indptr, const int32_t* indices, const uint32_t* rate, int64_t n, int64_t nnz, int32_t dim,
                          const double* y_in, double* y_out, void* scratch, size_t scratch_bytes, int64_t t0, int64_t t1,
                          int64_t total_epochs, double lr, double a, double b, double gamma, int32_t n_neg, uint64_t seed,
                          void* stream);
/* Placing NEW rows on a frozen map (the layout step of a UMAP transform): whisperseg_amd/embed.py::place_host is the definition and
 * embed.py::place the caller.  (indptr, indices, rate) is a CSR over the m new rows whose entries name CORPUS vertices 0 .. n - 1
 * (a row: at most 64 entries, nearest first); corpus: device float64 [n][dim], the frozen positions, only read; key: device uint64
 * [m], one per new row.  ONE launch runs the epochs t0 .. t1 - 1 of total_epochs, a lane per new row: in epoch t row i moves by
 * lr (1 - t / total_epochs) G_i, G_i the sum IN ROW ORDER over its entries q that are active in epoch t (the schedule above) of the
 * attraction term towards corpus[indices] and then the repulsion terms of the n_neg corpus vertices
 * ((mix(key[i] + ((t * 64 + q) * 16 + s)) >> 32) * n) >> 32, s = 0 .. n_neg - 1 — mix is splitmix64's finaliser; none is skipped.
 * A new row reads the corpus and itself only, so its result is a function of its own row, key and start: not of the other rows of
 * the call, their order or their number, nor of the grid.  With b == 1 every coordinate has the definition's bits.
 * m 0 .. 2^31 - 1 (m == 0 returns 0 without a launch), n 1 .. 2^31 - 1 where m > 0, nnz, dim, the epochs, n_neg and the parameters
 * as above.  An entry whose index is outside 0 .. n - 1 contributes nothing but keeps its position q, a row reaches no further than
 * 0 .. nnz and its entries past the 64th contribute nothing, so nothing outside the inputs is read whatever they hold.  y_in, y_out:
 * device float64 [m][dim]; y_out must overlap none of the inputs.  No scratch.  Every argument is validated on the host before the
 * launch (WSEG_ERR_INVALID, the argument's name in wseg_last_error()).  Stream-ordered, no host synchronisation.
 * Added without moving WSEG_ABI_VERSION (an addition). */
int wseg_embed_place_f64(const int64_t* indptr, const int32_t* indices, const uint32_t* rate, const uint64_t* key,
                         int64_t m, int64_t nnz, const double* corpus, int64_t n, int32_t dim,
                         const double* y_in, double* y_out, int64_t t0, int64_t t1, int64_t total_epochs,
                         double lr, double a, double b, double gamma, int32_t n_neg, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Principal components of float32 rows: the two heavy steps of whisperseg_amd/pca.py on the fp64 matrix cores
 * (v_mfma_f64_16x16x4_f64).  pca.py::moments_host and project_host are the definitions (numpy, float64); the covariance, the
 * eigen-decomposition and the conventions are host work there.
 *   wseg_pca_moments_f64   sum[c] = sum_n x[n][c] and gram[i][j] = sum_n x[n][i] x[n][j]: every product the exact float64 product
 *                          of the two float32 values, every sum within (n - 1) 2^-53 sum|terms| of its exact value and exact where
 *                          all partial sums are; gram is symmetric bit for bit (only the tiles on and above the diagonal are
 *                          computed).  The rows are split as a function of (n, d) alone and the partial tiles added in ascending
 *                          split order: no atomics, the same bits on every run.
 *   wseg_pca_project_f64   out[n][j] = sum_c (float64(x[n][c]) - mean[c]) basis[c][j], within (d + 2) 2^-53 sum|terms|.
 * rows: device float32 [n][d], finite; n 1 .. 2^31 - 1, d 1 .. 8192, r 1 .. 64.  sum: device float64 [d]; gram: device float64
 * [d][d]; mean: device float64 [d]; basis: device float64 [d][r], row-major; out: device float64 [n][r].  scratch: device, 8-byte
 * aligned, wseg_pca_scratch_bytes(n, d) bytes — host arithmetic, no device, monotone in n and d; 0 with the reason in
 * wseg_last_error() for sizes out of range.  Outputs and scratch must not overlap the inputs or each other.  Nothing outside rows,
 * mean and basis is read, nothing outside sum, gram, out and the scratch written.  Every argument is validated on the host before a
 * launch (WSEG_ERR_INVALID, the argument's name in wseg_last_error()).  Stream-ordered, no host synchronisation.
 * $WSEG_PCA_GRID: a TEST knob, the cap on the grids (the same bits for every value: the splits do not depend on it).
 * Added without moving WSEG_ABI_VERSION (an addition).
 * ---------------------------------------------------------------------------------------------- */
size_t wseg_pca_scratch_bytes(int64_t n, int32_t d);
int wseg_pca_moments_f64(const float* rows, int64_t n, int32_t d, double* sum, double* gram, void* scratch, size_t scratch_bytes,
                         void* stream);
int wseg_pca_project_f64(const float* rows, int64_t n, int32_t d, const double* mean, const double* basis, int32_t r, double* out,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * k nearest neighbours of every query row among the corpus rows under banded dynamic time warping, and the warping distance of
 * a list of pairs: the warping-tolerant counterpart of wseg_knn_f32 over the patches above or any float32 rows.  A row is a
 * sequence of `steps` columns of `channels` values, time fastest: row[ch * steps + t].  whisperseg_amd/dtw.py::dtw_host is the
 * definition (numpy, float64): the local cost c(a, b) = sum_ch (q[ch][a] - x[ch][b])^2, one sequential chain in ch with the
 * difference, the square and the addition each rounded once; G(0, 0) = c(0, 0), G(a, b) = c(a, b) + the least of G(a-1, b-1),
 * G(a-1, b), G(a, b-1) inside the band |a - b| <= band; dtw = G(steps-1, steps-1), no step weights, no normalisation; the
 * neighbours of row i are the k candidates that come first in the total order (dtw(i, j), j), ascending.  band == 0 is the squared
 * Euclidean distance.  The m x n matrix never exists: a selection kernel forms the costs |q_a|^2 + |x_b|^2 - 2 q_a.x_b of a tile of
 * pairs on the fp32 matrix cores (every term one channel-ordered fmaf chain: the same bits for every tiling, grid and split), runs
 * the recurrence over them in float32 and keeps the k + 8 best per row; a finish kernel recomputes those by the definition in
 * float64, orders them by (that distance as float32, j) and writes the first k — a reported distance has the definition's float32
 * bits, and the selection's error (<= 2 (2 steps - 1)(channels + 2 steps + 4) 2^-24 (max_a |q_a|^2 + max_b |x_b|^2)) only matters
 * at the k-th boundary.
 * queries: device float32 [m][channels * steps]; corpus: device float32 [n][channels * steps] (may be queries); m, n 0 .. 2^31 - 1,
 * channels 1 .. 128, steps 1 .. 64, band 0 .. steps - 1, k 1 .. 64.  exclude_same_index 1: j == i is no candidate (queries ==
 * corpus; by index, not by value).  Inputs must be finite; with non-finite input the order is unspecified, and still nothing
 * outside the outputs and scratch is written, nothing outside queries and corpus read.  index_out: device int32 [m][k];
 * distance_out: device float32 [m][k]; where a row has fewer than k candidates its tail is -1 / +inf.  scratch: device, 8-byte
 * aligned, wseg_dtw_scratch_bytes(m, n, channels, steps, k) bytes — host arithmetic, no device, monotone in m, n, steps and k; 0
 * with the reason in wseg_last_error() for sizes out of range.  m == 0 returns 0 without a launch; n == 0 only fills -1 / +inf.
 * wseg_dtw_pairs_f64: out[p] = float32(dtw(queries[pairs[p][0]], corpus[pairs[p][1]])) by the definition's float64 steps, for
 * pairs: device int32 [count][2], out: device float32 [count], count 0 .. 2^31 - 1 (0: no launch); a pair with an index outside its
 * rows reads nothing and gives NaN.
 * Every argument is validated on the host before a launch (WSEG_ERR_INVALID, the argument's name in wseg_last_error()).
 * Stream-ordered, no host synchronisation, no atomics.
 * $WSEG_DTW_GRID: a TEST knob, the cap on the grids and with it the candidate splits (the same bits for every value).
 * Added without moving WSEG_ABI_VERSION (an addition).
 * ---------------------------------------------------------------------------------------------- */
size_t wseg_dtw_scratch_bytes(int64_t m, int64_t n, int32_t channels, int32_t steps, int32_t k);
int wseg_dtw_knn_f32(const float* queries, int64_t m, const float* corpus, int64_t n, int32_t channels, int32_t steps, int32_t band,
                     int32_t k, int32_t exclude_same_index, void* scratch, size_t scratch_bytes, int32_t* index_out,
                     float* distance_out, void* stream);
int wseg_dtw_pairs_f64(const float* queries, int64_t m, const float* corpus, int64_t n, int32_t channels, int32_t steps, int32_t band,
                       const int32_t* pairs, int64_t count, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-segment fundamental frequency from the resident PCM: a YIN pitch contour of every row (what the spectral columns above do
 * not give: they name the loudest partial of a harmonic stack, not its fundamental, and nothing inside the call).
 * whisperseg_amd/pitch.py::frames_host is the definition (numpy, float64, every sum in a stated order); the kernel takes the same
 * float64 steps in the same order: the output has the definition's bits, on every run, for every workgroup size and grid.
 * bounds_host: HOST int64 [n_seg][2], the sample range [s0, s1) of every segment, 0 <= s0 <= s1 <= n (overlaps allowed; all time
 * arithmetic is the caller's).  pcm: device float32 [n].  2 <= tau_min < tau_max <= 2048, hop >= 1, 0 < threshold < 1.
 * Frame j of a segment starts at s0 + j hop and reads exactly 2 tau_max samples; a segment of len samples has 0 frames for
 * len < 2 tau_max, else 1 + (len - 2 tau_max) / hop: no padding, nothing at or behind s1 and nothing in front of s0 is ever read.
 * Per frame: d(tau) = sum_{i < tau_max} (x[i] - x[i + tau])^2 for tau = 1 .. tau_max, one sequential float64 chain per lag;
 * d'(tau) = (d(tau) tau) / run(tau) (1 where run is 0), run the prefix sum of d in blocks of 64 lags (sequential inside a block,
 * the bases the sequential sum of the block totals, run = base + inner); the lag is the first c in tau_min .. tau_max - 1 with
 * d'(c) < threshold walked up while d' falls (voiced), else the lowest minimiser of d' (unvoiced); period = lag + the vertex of the
 * parabola through d'(lag - 1 .. lag + 1), clamped to +-0.5 (0 where it has no minimum).
 * out: device float32 [total_frames][3], the frames of segment 0, then of segment 1, ...: (period in samples, d'(lag), voiced 0 / 1)
 * — RATE-FREE (no sampling rate enters the call).  Silence gives (tau_min, 1, 0).  Non-finite samples give unspecified values.
 * Nothing outside the total_frames rows is written.
 * scratch: device, 8-byte aligned, wseg_pitch_scratch_bytes(bounds_host, n_seg, tau_max, hop) bytes — host arithmetic, no device; it
 * returns 0 with the reason in wseg_last_error() for invalid bounds (it knows no n: s1 up to 2^52), n_seg < 0, tau_max outside
 * 3 .. 2048, hop < 1 or more than 2^40 frames.  (It holds the segment table the three per-segment calls share — int64 (s0, s1) of
 * every segment, then the exclusive prefix of the frame counts: 3 n_seg + 1 entries, padded to 256 bytes.  Size it by the query.)
 * The call copies what the kernel needs of the bounds through a pinned buffer of the library's on the stream and waits for
 * nothing: bounds_host may be reused on return.  n_seg == 0 or no frame at all returns 0 without a launch.  Every argument is
 * validated on the host before a launch (WSEG_ERR_INVALID, the argument's name in wseg_last_error()).  Stream-ordered.
 * $WSEG_PITCH_GRID: a TEST knob, the cap on the grid (the same bits for every value).
 * Added without moving WSEG_ABI_VERSION (an addition).
 * ---------------------------------------------------------------------------------------------- */
size_t wseg_pitch_scratch_bytes(const int64_t* bounds_host, int32_t n_seg, int32_t tau_max, int32_t hop);
int wseg_pitch_frames_f64(const float* pcm, int64_t n, const int64_t* bounds_host, int32_t n_seg,
                          int32_t tau_min, int32_t tau_max, int32_t hop, double threshold,
                          void* scratch, size_t scratch_bytes, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-segment signal-to-noise ratio from the resident PCM: how far a row lies above the recording's noise floor.
 * whisperseg_amd/snr.py holds the definition (numpy, float64).  Two calls, so that each stage can be pinned on its own.
 * wseg_frame_energy_f32: the band-energy track of a recording.  pcm: device float32 [n]; n_fft 512 .. 8192 (a power of two), hop =
 * n_fft / 4; window: device float32 [n_fft]; twiddle: device float32 [n_fft / 2][2] (W_n^k, 8-byte aligned), the log-mel
 * descriptor's.  WHOLE frames only: frame j = pcm[j hop : j hop + n_fft], J = wseg_frame_energy_frames(n, n_fft) = 0 for n < n_fft,
 * else 1 + (n - n_fft) / hop (host arithmetic; -1 with the reason in wseg_last_error() for an n_fft that is none or n outside
 * 0 .. 2^52) — no sample at or behind n is ever read.  track_out: device float32 [J], E[j] = sum_{k = k_lo .. k_hi}
 * |rfft(window * frame_j)[k]|^2, 0 <= k_lo <= k_hi <= n_fft / 2: the transform in fp32, the band sum in fp64 in a fixed order,
 * rounded to float32 once; the same bits on every run and for every grid.  Nothing outside the J values is written; J == 0 returns 0
 * without a launch.
 * wseg_snr_rows_f64: per row the mean and the maximum of its frames' energies and the noise floor of its window.  track: device
 * float32 [J], non-negative values, +inf and NaN (a NaN sorts last, as numpy.sort has it; negative values: unspecified).
 * table_host: HOST int64 [n_seg][3] = (j0, j1, window): the row's signal frames [j0, j1), 0 <= j0 <= j1 <= J, and the index of its
 * window in windows_host.  windows_host: HOST int64 [n_win][3] = (w0, w1, r): the frames [w0, w1), 0 <= w0 < w1 <= J, and the rank
 * 0 <= r <= w1 - w0 - 1.  All time arithmetic is the caller's.  Equal triples are selected once.
 * rows_out: device float64 [n_seg][3] = (S, M, N): S the float64 sum of the float32 energies of [j0, j1) over their count, M their
 * maximum (NaN if one is NaN), N = sort(track[w0:w1])[r] EXACTLY (a radix select over the bit patterns: integer counts only, the
 * same bits for every grid; a NaN floor is the quiet NaN); a row with j0 == j1 gets three NaN.
 * scratch: device, 8-byte aligned, wseg_snr_rows_scratch_bytes(J, table_host, n_seg, windows_host, n_win) bytes — host arithmetic,
 * no device; 0 with the reason in wseg_last_error() for invalid input.  The call copies its tables through a pinned buffer of the
 * library's on the stream and waits for nothing: both host arrays may be reused on return.  The number of launches depends on the
 * windows' lengths only, never on the track's values.  n_seg == 0 returns 0 without a launch.  Every argument is validated on the
 * host before a launch (WSEG_ERR_INVALID, the argument's name in wseg_last_error()).  Stream-ordered, no host synchronisation.
 * $WSEG_SNR_GRID: a TEST knob, the cap on the grids (the same bits for every value).
 * Added without moving WSEG_ABI_VERSION (an addition).
 * ---------------------------------------------------------------------------------------------- */
int64_t wseg_frame_energy_frames(int64_t n, int32_t n_fft);
int wseg_frame_energy_f32(const float* pcm, int64_t n, int32_t n_fft, int32_t k_lo, int32_t k_hi, const float* window,
                          const float* twiddle, float* track_out, void* stream);
size_t wseg_snr_rows_scratch_bytes(int64_t J, const int64_t* table_host, int32_t n_seg, const int64_t* windows_host, int32_t n_win);
int wseg_snr_rows_f64(const float* track, int64_t J, const int64_t* table_host, int32_t n_seg, const int64_t* windows_host,
                      int32_t n_win, void* scratch, size_t scratch_bytes, double* rows_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whisper encoder-decoder.
 * Replaces HF WhisperForConditionalGeneration as the reference drives it:
 *   construction  reference model.py:626-644 (WhisperSegmenter.__init__, from_pretrained)
 *   generate      reference model.py:647-676 / 604-622 (model.generate(...) per batch)
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t d_model, n_heads, enc_layers, dec_layers, ffn, vocab;
  int32_t n_mels;           /* 80   */
  int32_t spec_cols;        /* total_spec_columns: 2 * enc_positions, 256 .. 3000 (default 1000; reference train.py:72) */
  int32_t enc_positions;    /* spec_cols / 2 = 128 .. 1500 rows of Whisper's position table (default 500; reference model.py:76-86) */
  int32_t dec_positions;    /* 448  */
  int32_t dtype;            /* wseg_dtype: arithmetic/storage type of weights and activations */
} wseg_model_config;

typedef struct wseg_model wseg_model;

int wseg_model_create(const wseg_model_config* cfg, wseg_model** out);
void wseg_model_destroy(wseg_model* m);
/*
 * Attach one prepared weight tensor (device pointer, caller-owned, must outlive the model).
 * Names and layouts are listed in whisperseg_amd/engine.py::prepare_weights (e.g. "enc.0.qkv.w"
 * = [3*d_model, d_model] row-major in the model dtype).  bytes is checked against the expected size.
 */
int wseg_model_set_tensor(wseg_model* m, const char* name, const void* dev_ptr, size_t bytes);
/* 0 when every tensor the geometry needs has been attached. */
int wseg_model_ready(const wseg_model* m);

/* Workspace (device bytes) for max_windows window slots (= windows decoded concurrently; the encoder runs over at most 256 of
 * them per pass, fewer when enc_positions > 512: about 131 072 / enc_positions, a function of the geometry alone).
 *
 * The decoder's self-attention K / V are PAGED (ABI 5): pages of 8 positions are handed to a slot as its sequence grows and taken
 * back when its window retires, from a pool carved out of the workspace.  wseg_workspace_bytes sizes that pool for the EXPECTED
 * sequence length — min(max_length, 64) positions per slot on average — so the reference's default max_length = 448
 * (model.py:406-409) no longer reserves 448 positions per slot up front (1.3 MiB per position per slot in the split-precision
 * modes); wseg_workspace_bytes_kv takes the average number of positions per slot to provision (0: that default; >= max_length:
 * every slot can reach max_length at once, the pre-ABI-5 behaviour).  wseg_generate uses whatever the caller's workspace has room
 * for (at most a full set, at least one slot's worth); when the pool runs short it preempts the youngest window and decodes it
 * again later (same tokens; wseg_generate_stats.n_preemptions). */
size_t wseg_workspace_bytes(const wseg_model* m, int32_t max_windows, int32_t num_beams, int32_t max_length);
size_t wseg_workspace_bytes_kv(const wseg_model* m, int32_t max_windows, int32_t num_beams, int32_t max_length,
                               int32_t kv_positions_per_slot);

/*
 * Encoder only: feats device float32 [n_windows][n_mels][spec_cols] -> enc_out device [n_windows][enc_positions][d_model]
 * in the model dtype.  (HF modeling_whisper.py:592-646 as reached from reference model.py:655.)
 */
int wseg_encode(wseg_model* m, const float* feats, int32_t n_windows,
                void* workspace, size_t workspace_bytes, void* enc_out, void* stream);

typedef struct {
  int32_t prompt[8];              /* decoder_input_ids, reference model.py:656 */
  int32_t prompt_len;
  int32_t eos_token_id, pad_token_id;   /* reference model.py:658-659 */
  int32_t max_length;             /* total length incl. prompt (HF 4.38.2 semantics), model.py:660 */
  int32_t num_beams;              /* 1 = greedy (do_sample with top_k=1, model.py:662-663), else beam search */
  float length_penalty;           /* model.py:665 */
  const int32_t* suppress_tokens; /* device [n_suppress]   generation_config.suppress_tokens        */
  int32_t n_suppress;
  const int32_t* begin_suppress_tokens; /* device [n_begin_suppress] applied at the first generated position */
  int32_t n_begin_suppress;
  /* In-flight batching (the reference decodes batch by batch, model.py:653, one file at a time,
   * scripts/segment.py:39-56).  0 selects the default of each. */
  int32_t n_slots;                /* window slots decoded concurrently; 0 or >= n_windows: one per window                */
  int32_t refill_min;             /* admit queued windows once this many slots are free; 0: n_slots / 8 (min 1)         */
  int32_t lookahead;              /* decode steps the host may run ahead of the device; 0: 1                            */
  const int32_t* window_max_length; /* device [n_windows] per-window cap on the total length (clamped to max_length), or
                                     NULL: every window may run to max_length                                           */
  /* Sampling (reference model.py:615-616, 662-663: do_sample = (num_beams == 1) with top_k / top_p).  Used only when
   * num_beams == 1 and top_k > 1: the next token is drawn from softmax over the top_k processed logits, further cut to the
   * nucleus top_p (HF TopKLogitsWarper then TopPLogitsWarper), with a counter-based generator keyed by (seed, window,
   * position) — reproducible for a seed, but not the torch generator stream HF would consume.  top_k <= 1: argmax. */
  int32_t top_k;                  /* 0 / 1: deterministic argmax (the reference's default top_k = 1); 2..16: sample       */
  float top_p;                    /* nucleus mass in (0, 1]; values <= 0 or >= 1 disable the cut                          */
  uint64_t seed;
  const void* encoder_output;     /* device [n_windows][enc_positions][d_model] in the model dtype: precomputed encoder
                                     states (wseg_encode) used instead of running the encoder on feats (feats may then
                                     be NULL; rows past the last window must be readable up to a multiple of 256 — and, when
                                     enc_positions > 512, for 256 rows more: the shorter encoder passes of such a geometry
                                     need not start on a multiple of 256 rows), or NULL */
} wseg_generate_params;

/*
 * Full decode of n_windows windows: encoder, cross-K/V, then greedy / beam search with HF semantics
 * (generation/utils.py:3208-3510), entirely on device.
 *   out_tokens  device int32 [n_windows][max_length]  best sequence INCLUDING the prompt, pad-filled
 *   out_lengths device int32 [n_windows]              number of valid tokens (prompt + generated)
 * The windows are decoded through n_slots window slots: a slot whose window has finished (EOS / early-stop heuristic /
 * max_length) is retired and re-used for the next queued window while the other slots keep decoding, every slot at its
 * own position.  Idle slots are skipped by every per-step kernel.  The workspace is sized by
 * wseg_workspace_bytes(m, n_slots, ...): it does not grow with n_windows.  The host stays `lookahead` steps ahead of the
 * device and otherwise only waits on the small per-step status mirror; the call is stream-ordered on `stream`.
 * (ABI 3 had decode "lanes" — slot groups on separate streams; they measured exactly as one group with their total slot
 * count and were removed in ABI 4.  ABI 5: paged self-attention K / V, see wseg_workspace_bytes.)
 */
int wseg_generate(wseg_model* m, const float* feats, int32_t n_windows, const wseg_generate_params* p,
                  void* workspace, size_t workspace_bytes,
                  int32_t* out_tokens, int32_t* out_lengths, void* stream);

/* Scheduler statistics of the last wseg_generate call on this model. */
typedef struct {
  int32_t n_windows, n_slots;
  int32_t n_steps;                /* decode steps launched (each steps every active slot once)                          */
  int32_t n_admissions;           /* encoder + cross-K/V passes (groups of windows admitted into free slots)            */
  int64_t slot_steps_active;      /* sum over steps of slots that were decoding a window                                */
  int64_t slot_steps_total;       /* steps * slots                                                                      */
  int64_t queued_slot_steps_active; /* the same two sums over the steps launched while windows were still queued, i.e.   */
  int64_t queued_slot_steps_total;  /* without the drain of the last windows (steady-state occupancy of the refill)      */
  int32_t kv_units_total;         /* self-attention K/V pool of the call: units of (one 8-position page x all beams of a slot) */
  int32_t kv_units_peak;          /* most units in use at once                                                           */
  int32_t n_preemptions;          /* windows aborted for lack of pool units and decoded again later                       */
  int32_t reserved_;
} wseg_generate_stats;
int wseg_last_stats(const wseg_model* m, wseg_generate_stats* out);

/* WSEG_F16M6: GEMM operand rows of the mixed split-precision mode from WSEG_F16X3 operand rows (whisperseg_amd/engine.py::
 * split_operand with IEEE-half pairs).  src: device, rows of 2 K 16-bit words; dst: device, rows of 4 K bytes (must not alias
 * src); K % 64 == 0.  weight_order != 0 for the W operand of a GEMM (weight matrices: what wseg_model_set_tensor expects in
 * WSEG_F16M6 mode), 0 for an activation operand (only the library's own GEMM wrappers and wseg_debug_gemm need that). */
int wseg_convert_operand(const void* src_x3_rows, void* dst_m6_rows, int64_t n_rows, int32_t K, int32_t weight_order, void* stream);

/* Debug/parity taps (used by tests): first-step logits fp32 [n_windows*num_beams][vocab] of the last
 * wseg_generate call are kept in the workspace; this copies them out (device to device). */
int wseg_debug_first_logits(wseg_model* m, void* workspace, float* out, int32_t n_rows, void* stream);

/* Debug/parity tap: logits and decode state of CHOSEN decode steps of a wseg_generate call (tests/test_late_step_logits_gpu.py
 * compares them with a float64 oracle fed the engine's own row histories).  A step is named by the position its slots feed: the
 * self-attention of that step sees position + 1 keys, the first generated step is prompt_len - 1, the last one max_length - 2.
 *   arm     positions[n_steps]: ascending, n_steps <= 16 (0 disarms); out: device buffer of n_steps records, filled in the order of
 *           `positions`.  Holds for the NEXT wseg_generate call on this model only — the parameters struct does not change — and
 *           `out` must stay valid until that call's stream work has completed.  Steps the call never reaches write nothing.
 *   record  for S = min(n_slots, n_windows) slots, nb beams, R = S * nb rows (row = slot * nb + beam; window i sits in slot i),
 *           L = max_length, V = vocab, back to back:
 *             float   logits[R][V]    as the LM head wrote them: before suppression / log-softmax, like wseg_debug_first_logits
 *             int32_t run_seq[R][L]   token history of every row; entries 0 .. position are the tokens fed so far
 *             int32_t pos[S]          position of every slot
 *             int32_t idle[S]         1 = the slot was idle (its window had finished) and the step skipped it
 *             uint8_t anc[R][L]       ancestry: the beam whose cache rows hold position p of the row's history (rounded up to 4 bytes)
 *           all as they were when the step ran (before its beam / greedy bookkeeping).  wseg_debug_step_snapshot_bytes: bytes of one record.
 *   result  after the call: *n_taken = records written; *qkv_split (may be NULL) = 1 when the snapshot steps' q | k | v GEMM handed
 *           split-K partials to the self-attention kernel (which finishes the reduction and appends K / V itself), 0 when the GEMM
 *           epilogue wrote q and the cache rows, -1 when no snapshot step ran in the decode loop.  WSEG_ERR_STATE unless the call
 *           was armed, all its windows started together (n_slots >= n_windows) and none was preempted.
 * A snapshot step is launched eagerly, every other step still replays the step graph; the call computes exactly what it computes
 * without a snapshot (same kernels, same order).  These entry points were added without moving WSEG_ABI_VERSION: the version
 * moves when an existing declaration changes its layout or meaning (ABI 3 -> 4 -> 5 above), not when a tap is added. */
size_t wseg_debug_step_snapshot_bytes(const wseg_model* m, int32_t n_slots, int32_t num_beams, int32_t max_length);
int wseg_debug_step_snapshot_arm(wseg_model* m, const int32_t* positions, int32_t n_steps, void* out, size_t out_bytes);
int wseg_debug_step_snapshot_result(const wseg_model* m, int32_t* n_taken, int32_t* qkv_split);

/* Host-only tap (no model, no workspace, no device; tests/test_scheduler_cpu.py): runs wseg_generate's slot scheduler — the very
 * object the call drives — against a SCRIPTED device.  Inputs are the scheduler's resolved geometry: window slots, pool units,
 * max_length, npf = prompt positions the admission's pass covers, pos0 = the position a slot is at when the decode loop first steps
 * it (wseg_generate uses (0, 0), (P, P) or (min(P - 1, 4), the same)), refill_min / lookahead as in wseg_generate_params, and
 * done_after[n_windows]: the decode-loop steps after which the window's slot reports done (0: it ended inside the admission's pass).
 * Writes the statistics such a call would report and a trace of int32 records (kind, a, b, c), in the order the work would be enqueued:
 *   1 admit    (slot, window, 0)
 *   2 assign   (slot, page, unit)       after the admission / before the step it belongs to; only pairs that reach the device
 *   3 preempt  (slot, 0, 0)             before the assignments of its step
 *   4 step     (t, 0, 0)
 *   5 retire   (slot, u, 0)             u: the step whose status showed the slot done
 * *trace_len = int32 entries of the whole trace; trace may be NULL (count only), otherwise trace_cap entries must hold it.
 * Scheduler errors (WSEG_ERR_STATE) are those of wseg_generate. */
int wseg_debug_sched_trace(int32_t n_windows, int32_t n_slots, int32_t kv_units, int32_t max_length, int32_t npf, int32_t pos0,
                           int32_t refill_min, int32_t lookahead, const int32_t* done_after, wseg_generate_stats* stats,
                           int32_t* trace, int64_t trace_cap, int64_t* trace_len);

/* Model-free tap of ONE decode step's token selection (tests/test_decode_step_gpu.py): on caller-provided device memory it runs
 * exactly what a decode step of wseg_generate runs after the LM head has written its logits, with the library's own launchers:
 *   1. the suppress mask from the two lists (ids < 0 or >= vocab are ignored);
 *   2. per row: log-softmax, suppression (-inf; the begin list only when the row's length equals prompt_len), + running beam
 *      score, top-Kc (Kc = 2 num_beams; greedy: 1, sampling: top_k, and then the RAW processed logits, no log-softmax).  The
 *      vocabulary is cut into clamp(ceil(512 / (n_slots * num_beams)), 1, 16) slices of ceil(vocab / slices) ids.  Equal values:
 *      the lower id wins, within a slice, across slices and across beams;
 *   3. HF's _beam_search bookkeeping (num_beams > 1) or the greedy choice / the sampler (num_beams == 1);
 *   4. when out_tokens / out_lengths are given: the retirement of the slots this step finished (done 0 -> 1), into row win[slot].
 * The sampler (num_beams == 1, top_k > 1), so that a reference can restate it: pr[j] = expf(v[j] - v[0]) over the top_k candidates,
 * best first (fp32; a suppressed candidate has weight 0); candidates are kept from j = 0 while pr[j] > 0 and (with 0 < top_p < 1)
 * the weight before j is < top_p * sum(pr); x = seed + 0x9E3779B97F4A7C15 * (window * 4096 + cur_len + 1) mod 2^64, cur_len = pos + 1
 * tokens present; the splitmix64 finaliser x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27, x *= 0x94D049BB133111EB,
 * x ^= x >> 31; u = float(x >> 40) * 2^-24 * (kept weight); the drawn candidate is the first whose cumulated weight (fp32, in
 * order) exceeds u, the last kept one if none does.
 * State arrays (device, read and written in place; S = n_slots, R = S * num_beams rows, row = slot * num_beams + beam,
 * L = max_length), as wseg_generate keeps them:
 *   int32 [S]     pos (position of the token the slot fed: pos + 1 tokens are present), done (1: idle, every kernel skips the slot),
 *                 win (window index: the sampler's key and the output row), wmax (cap on the total length), unsat
 *   [R]           int32 tokens_in, float run_score, float fin_score, int32 fin_flag, int32 fin_len
 *   [R][L]        int32 run_seq, int32 fin_seq, uint8 anc
 *   [R][Kc]       float cand_val, int32 cand_tok: the step's candidates per row, best first (room for [R][16] always suffices)
 * logits: device fp32 [rows][ldv], 16-byte aligned, columns >= vocab are never read.  list == NULL: rows = R, every slot that is not
 * done is stepped.  list != NULL (device, n_list distinct slots; the admission's form): only those slots, logits row i is the ONE
 * row of slot list[i] shared by its beams, and the vocabulary is sliced as for the whole population of n_slots.
 * scratch: device, 256-byte aligned, wseg_debug_decode_step_scratch_bytes (0 for an unsupported geometry).  out_tokens
 * [n_out_rows][L] / out_lengths [n_out_rows]: both or neither (then n_out_rows = 0).
 * Every argument is checked on the host before anything is launched (WSEG_ERR_INVALID, the argument's name in wseg_last_error());
 * then pos / done / win and the list are read back and refused alike when a stepped slot's pos + 1 >= max_length, its win is
 * negative or past the output rows, or a list entry is no slot or repeats.  The call synchronises the stream.  Not covered by this
 * tap: the LM head, the slot scheduler and the replay of the step graph. */
typedef struct {
  int32_t n_slots, num_beams;     /* num_beams 1..8 */
  int32_t max_length;             /* L: total length incl. prompt, capacity of the sequence arrays */
  int32_t vocab, ldv;             /* ldv >= vocab, ldv % 4 == 0 */
  int32_t prompt[8];
  int32_t prompt_len;             /* 1..8, < max_length */
  int32_t eos_token_id, pad_token_id;
  float length_penalty;
  int32_t top_k;                  /* 0..16; used when num_beams == 1: 0 / 1 argmax, else sample */
  float top_p;
  uint64_t seed;
  const int32_t* suppress_tokens; /* device [n_suppress] */
  const int32_t* begin_suppress_tokens; /* device [n_begin_suppress] */
  int32_t n_suppress, n_begin_suppress;
} wseg_decode_step_params;
typedef struct {
  int32_t *pos, *done, *win, *wmax, *unsat;
  int32_t* tokens_in;
  float *run_score, *fin_score;
  int32_t *fin_flag, *fin_len;
  int32_t *run_seq, *fin_seq;
  uint8_t* anc;
  float* cand_val;
  int32_t* cand_tok;
} wseg_decode_step_state;
size_t wseg_debug_decode_step_scratch_bytes(int32_t n_slots, int32_t num_beams, int32_t vocab);
int wseg_debug_decode_step(const wseg_decode_step_params* p, const wseg_decode_step_state* state, const float* logits,
                           const int32_t* list, int32_t n_list, void* scratch, size_t scratch_bytes, int32_t* out_tokens,
                           int32_t* out_lengths, int32_t n_out_rows, void* stream);

/* Per-stage device time (ms) of the last wseg_generate call on this model, measured with HIP events
 * on the call's stream: [0]=encoder passes, [1]=cross-K/V passes, [2]=everything else (the decode steps),
 * [3]=number of decode steps. */
int wseg_last_timing(const wseg_model* m, float out[4]);

/* Test / tuning tap: out[M][N] = epilogue(A[M][K] * W[N][K]^T + bias) with the library's GEMM of the given dtype.
 * epi: 0 store, 1 GELU, 2 residual add (resid[M][N] and out are the fp32 residual stream in every dtype).  A must have
 * round_up(M,256) readable rows, N % 128 == 0,
 * K % 64 == 0.  Used by tests/test_gemm_gpu.py (parity vs torch / fp64) and tools/gemm_bench.py. */
int wseg_debug_gemm(int32_t dtype, int32_t epi, int32_t M, int32_t N, int32_t K, const void* A, const void* W,
                    const void* bias, const void* resid, void* out, void* splitk_ws, size_t splitk_ws_bytes, void* stream);

/* WSEG_F16M6: 1 when wseg_debug_gemm with epi 0 / 1 writes its output as M6 rows (the LDS-staged epilogues of the large-tile
 * kernels; the skinny family when it splits K — assumed here: a workspace that never limits the split), 0 when it writes hi | lo
 * IEEE-half rows (skinny family, K not split); always 0 for the other dtypes. */
int wseg_debug_gemm_out_is_mx(int32_t dtype, int32_t M, int32_t N, int32_t K);

/* Test / tuning tap of the decoder's fused step x += A W^T + bias; y = LayerNorm(x) * gamma + beta (x: fp32 residual stream [M][N],
 * in place; y: GEMM operand rows of the dtype; bias / gamma / beta: parameter type of the dtype).  Same operand rules as
 * wseg_debug_gemm.  Used by tests/test_gemm_gpu.py and tools/gemm_bench.py --resid-ln. */
int wseg_debug_gemm_resid_ln(int32_t dtype, int32_t M, int32_t N, int32_t K, const void* A, const void* W, const void* bias, void* x,
                             const void* gamma, const void* beta, void* y, void* splitk_ws, size_t splitk_ws_bytes, void* stream);

/* Model-free taps of the decode step's cross-attention and of the K / V rows it reads (tests/test_cross_attn_gpu.py,
 * oracle/cross_kv.py): caller-owned device memory, no model, no workspace plan, no arithmetic of their own.  d = 64 n_heads.
 *
 * wseg_debug_cross_kv_bytes (host only): bytes of ONE cross K (or V) buffer of n_slots slots and, in *format (may be NULL), the
 * storage the mode takes at this beam count: 0 plain rows [slot][head][t_len][64] (fp32 in the split modes), 2 / 3 the packed
 * block-floating-point rows (132 / 196 bytes per (position, head) row).  0 with the reason in wseg_last_error() for an
 * unsupported geometry.
 *
 * wseg_debug_cross_kv: the cross K / V projection of one decoder layer exactly as the encode pass of wseg_generate launches it:
 * k | v = a w^T + bias through the library's GEMM with the K / V epilogue, rows of window i into slot slot_map[i] (NULL: slot i).
 *   a         operand rows of the mode [n_windows * t_len][d] (fp32 / 16-bit rows; hi | lo rows; M6 rows), a_bytes must cover
 *             the row count rounded up to 256
 *   w, bias   weight operand rows [2 d][d] (M6: weight order) and the bias [2 d] in the mode's parameter type (NULL: none)
 *   slot_map  device [n_windows], distinct slots; read back and checked before the launch
 *   plan_m    the row count the launch is PLANNED for (>= the rows launched; wseg_generate: a whole encoder chunk), which fixes the
 *             kernel family and with it the summation order
 *   k, v      device buffers of kv_bytes >= wseg_debug_cross_kv_bytes each; splitk_ws: the GEMM's split-K workspace (the packed rows
 *             need it whenever the plan is the weight-stream family)
 *
 * wseg_debug_cross_attention: the decode step's cross-attention launcher on such buffers.  Query row r = window * num_beams + beam;
 * window w reads the K / V of slot kv_slot[w] (NULL: slot w; the map exists for the packed rows only).  The query is given either
 *   q         finished, pre-scaled rows [R][d] in the mode's plain type (fp32; 16-bit in WSEG_BF16 / WSEG_F16), or
 *   q_part    split-K partial planes fp32 [q_splits][m_pad][d], m_pad >= R, which the kernel sums in plane order, adds q_bias [d]
 *             (may be NULL) to and multiplies by `scale` (not WSEG_F32).
 * done: device [n_windows], 1 = the window is idle and its output rows stay untouched.  out: [R][d] in the mode's operand format
 * (fp32 / 16-bit rows, hi | lo rows, M6 rows from the 16-bit block-floating-point kernel), out_bytes must cover it.
 *
 * Both taps check every argument on the host before anything is launched (WSEG_ERR_INVALID, the argument's name in
 * wseg_last_error()) and synchronise the stream.  Not covered by them: the co-proj GEMM behind the attention, the scheduler's
 * admission and the replay of the step graph. */
size_t wseg_debug_cross_kv_bytes(int32_t dtype, int32_t num_beams, int32_t n_slots, int32_t n_heads, int32_t t_len, int32_t* format);
int wseg_debug_cross_kv(int32_t dtype, int32_t num_beams, int32_t n_windows, int32_t n_slots, int32_t t_len, int32_t n_heads,
                        int32_t plan_m, const void* a, size_t a_bytes, const void* w, const void* bias, const int32_t* slot_map,
                        void* k, void* v, size_t kv_bytes, void* splitk_ws, size_t splitk_ws_bytes, void* stream);
int wseg_debug_cross_attention(int32_t dtype, int32_t num_beams, int32_t n_windows, int32_t n_slots, int32_t t_len, int32_t n_heads,
                               const void* q, const float* q_part, int32_t q_splits, int32_t m_pad, const void* q_bias, float scale,
                               const int32_t* done, const int32_t* kv_slot, const void* k, const void* v, size_t kv_bytes, void* out,
                               size_t out_bytes, void* stream);

/* Test tap of the cross-lane exchanges every wave reduction of the library is built on (csrc/wseg_common.h lane_xor<M>: DPP
 * quad_perm / row_shl / row_shr / row_ror, v_permlane16_swap, v_permlane32_swap instead of ds_bpermute): out[m][l] = the value
 * lane l ^ (1 << m) holds, for m = 0..5 and l = 0..63, where lane l holds 7 l + 3.  out: device, 6 * 64 uint32.
 * tests/test_gemm_gpu.py::test_lane_exchanges. */
int wseg_debug_lane_xor(uint32_t* out, void* stream);

/* Live per-launch timing of the dominant kernel (the 256x256 ping-pong bf16 MFMA GEMM; 128x128 persistent for narrow problems) with HIP events recorded on
 * the launching stream.  Between begin and end every launch of that kernel is bracketed by two events;
 * end synchronises and returns the sums: algorithmic FLOPs (2*M*N*K of the real, un-padded problem),
 * kernel milliseconds and the number of launches.  Process-wide; intended for bench.py's roofline leg. */
int wseg_profile_begin(void);
int wseg_profile_end(double* total_flops, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* WSEG_H */
