/* zafx.h -- C-ABI of libzafx.so: MI355X (gfx950) kernels for the windowed-transform
 * hot path of zafarrafii/Zaf-Python (zaf.py).
 *
 * The reference has no FFI: its boundary is the Python signatures of zaf.py.  This
 * header is the boundary the reference-side binding (a ctypes stub)
 * binds instead of NumPy/SciPy for each call site below.  Plain C types only; no
 * exceptions cross; every function returns 0 on success or a non-zero code whose
 * text is available from zafx_last_error() (thread-local).
 *
 *   entry point / plan kind        replaces (zaf.py file:line)
 *   -----------------------------  -------------------------------------------------
 *   ZAFX_STFT                      stft            zaf.py:45-141  (np.pad :112, frame
 *                                                  loop :132-136, np.fft.fft :139)
 *   ZAFX_ISTFT                     istft           zaf.py:144-243 (np.fft.ifft :223,
 *                                                  overlap-add :226-233, trim :236, gain :241)
 *   ZAFX_MEL                       melspectrogram  zaf.py:324-375 (stft :369, abs :370,
 *                                                  np.matmul :373)
 *   ZAFX_MFCC                      mfcc            zaf.py:378-454 (power :437, matmul+log
 *                                                  :443-446, scipy.fftpack.dct :443-449)
 *   ZAFX_CQT                       cqtspectrogram  zaf.py:562-635 (np.pad :612, np.fft.fft
 *                                                  + CSR mat-vec + abs :630-632)
 *   ZAFX_CHROMA                    cqtchromagram   zaf.py:638-700 (strided row sums :693-698)
 *   ZAFX_MDCT                      mdct            zaf.py:984-1075 (per-frame FFT :1061-1073)
 *   ZAFX_IMDCT                     imdct           zaf.py:1078-1184 (FFT :1159, TDAC
 *                                                  overlap-add :1172-1179, trim :1182)
 *   ZAFX_DCT                       dct / dst       zaf.py:703-839, :842-981 (np.fft.fft of the 2N-2 /
 *                                                  2N+2 / 4N / 8N point extension :771, :791, :816, :834,
 *                                                  :909, :926, :948, :974; orthonormal scalings)
 *   ZAFX_CENTER / _CENTER_SIDES    the center / sides example of istft's docstring, zaf.py:155-198 (stft of both
 *                                  channels :176-177, magnitudes :181-182, masks :185-186, masked spectra :190-191,
 *                                  istft :194-195, sides :198) in one kernel
 *   ZAFX_MASKFILTER / _REST with   the same example with a mask of the caller's: stft zaf.py:176-177, the mirrored real mask times the
 *   zafx_execute_masked            spectrum :190-191 (np.concatenate((mask, mask[-2:0:-1])) * audio_stft), istft :194-195 and, _REST,
 *                                  the subtraction :198, for a mono clip in one kernel; zafx_plan_mask_dims gives the mask's shape
 *                                  (clips of different lengths in one launch: zafx_execute_masked_ragged, zafx_plan_mask_ragged_layout;
 *                                  several masks per clip over one forward transform: zafx_execute_masked_stems;
 *                                  both at once: zafx_execute_masked_stems_ragged, zafx_plan_stems_ragged_layout)
 *   ZAFX_MASKFILTER / _REST with   the same with a COMPLEX mask, extended to its Hermitian mirror:
 *   zafx_execute_masked_complex    np.concatenate((M, np.conj(M[-2:0:-1]))) * audio_stft, istft :194-195 (the real part, :223); complex64
 *                                  masks in ZAFX_LAYOUT_TF; clips of different lengths in one launch: zafx_execute_masked_complex_ragged
 *   ZAFX_MASKFILTER / _REST with   the same for an interleaved stereo clip (N, 2), as the example has it: one real mask for both channels
 *   zafx_execute_masked_stereo     or one per channel, masks in ZAFX_LAYOUT_TF; clips of different lengths in one launch:
 *                                  zafx_execute_masked_stereo_ragged, zafx_plan_stereo_ragged_layout
 *   ZAFX_MASKFILTER / _REST with   zafx_execute_masked (n_channels 1, masks in ZAFX_LAYOUT_TF) and zafx_execute_masked_stereo (2) on 16-bit PCM:
 *   zafx_execute_masked_pcm        int16 samples in, s / 32768 (wavread, zaf.py:1202), int16 or float32 samples out; clips of different
 *                                  lengths in one launch: zafx_execute_masked_pcm_ragged
 *   zafx_plan_set_constant         operands built by melfilterbank zaf.py:246-321 and
 *                                  cqtkernel zaf.py:457-559 (scipy.sparse CSR, consumed
 *                                  at zaf.py:373, :445, :631)
 *
 * Ownership: host buffers belong to the caller; device buffers belong to whoever
 * called zafx_alloc; a plan owns its HIP stream, events, twiddle tables and constants.
 * Threading: a plan is bound to one device and one stream; calls on distinct plans
 * are thread-safe; calls on one plan must be serialised by the caller.
 * All device arrays are float32 / complex64 (interleaved re,im), C-contiguous -- float64 /
 * complex128 for plans created with ZAFX_PRECISION_F64.
 * A device array may start anywhere on the grid of its real type -- 4 bytes for the float32 kinds (complex64
 * included: 4, not 8), 8 for the float64 ones (complex128 included), 2 for int16 and 4 for int32 PCM --, e.g. a slice
 * of a batch or a piece of an arena; the fast routes additionally want the base on a 128-byte line (what zafx_alloc
 * returns), other bases run on slower forms of the same kernels or on the generic ones (zafx_plan_last_kernel_name).
 * Nothing outside the arrays is read into a result or written: not the bytes in front of element 0, not those behind
 * the last element, not the row padding of a row_align plan, and no clip's result depends on another clip's samples.
 */
#ifndef ZAFX_H
#define ZAFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZAFX_VERSION 101

typedef struct zafx_plan zafx_plan;
typedef struct zafx_comm zafx_comm;

enum zafx_kind {
    ZAFX_STFT = 1,   /* in (B, N) f32            -> out (B, W, T) c64 [FT] or (B, T, W) [TF]       */
    ZAFX_ISTFT = 2,  /* in (B, W, T)/(B, T, W)   -> out (B, T*H - (W-H)) f32    (one-sided: W/2+1 rows) */
    ZAFX_MDCT = 3,   /* in (B, N) f32            -> out (B, W/2, T) f32 [FT] or (B, T, W/2) [TF]   */
    ZAFX_IMDCT = 4,  /* in (B, W/2, T)/(B,T,W/2) -> out (B, (W/2)*(T-1) - 1) f32                   */
    ZAFX_MEL = 5,    /* in (B, N) f32            -> out (B, n_filters, T) or (B, T, n_filters)     */
    ZAFX_MFCC = 6,   /* in (B, N) f32            -> out (B, n_coefs, T)   or (B, T, n_coefs)  (with_mel: n_filters + n_coefs rows) */
    ZAFX_CQT = 7,    /* in (B, N) f32            -> out (B, n_bins, T)    or (B, T, n_bins)        */
    ZAFX_CHROMA = 8, /* in (B, N) f32            -> out (B, octave_resolution, T) or transposed    */
    ZAFX_LINEAR = 9, /* in (B, window_length) f32 -> out (B, n_filters) f32: y = M x per clip (a caller's own dense
                        map; dct / dst lengths the FFT form below does not take)                          */
    ZAFX_DCT = 10,   /* in (B, N) f32 -> out (B, N) f32: the orthonormal dct / dst of zaf.py:703-839 / :842-981, type
                        params.transform_type = 1..4, params.transform_sine = 0 (dct) / 1 (dst), N = window_length;
                        one M-point complex FFT per vector where M = N/2 (N-1 / N+1 for type I) is a power of two 32..8192,
                        every other N from 2 to 8192 on Bluestein convolutions: types 2-4 of N = 4 j two transforms of
                        2^ceil(log2(N-1)) points around the N/2-point transform, the rest two of 2^ceil(log2(2N-1)) (chirp-z sum) */
    ZAFX_CENTER = 11,       /* in (B, N, 2) f32, interleaved stereo as wavread returns it -> out (B, N, 2) f32: the center of zaf.py:155-198,
                               center[:, c] = istft(concat(m_c, m_c[-2:0:-1]) * stft(x[:, c]))[0:N] with the masks m_0 = (b < a) ? b / a : 1,
                               m_1 = (a < b) ? a / b : 1 of a = |stft(x[:, 0])|, b = |stft(x[:, 1])| on rows 0..W/2.  The masks equal the
                               reference's min(a, b) / a wherever that is finite; where the reference divides 0 by 0 (an exactly silent bin,
                               which it turns into a frame of NaNs) the masked bin is 0, the limit value -- the one deliberate departure.
                               float32 only, window_length 256 / 512 / 1024 / 2048, step_length = window_length / 2 (zaf.stft pads W/2 in
                               front and zaf.istft trims W - H: at any other hop the reference's example fails on a shape mismatch);
                               n_in = N sample frames; zafx_plan_out_dims: dims[0] = sample frames written per clip, dims[1] = 2 */
    ZAFX_CENTER_SIDES = 12, /* as ZAFX_CENTER -> out (B, 2, N, 2): block 0 of a clip the center, block 1 the sides = input - center (:198);
                               the center is bit-identical to ZAFX_CENTER's.  Neither kind takes zafx_execute_ragged, zafx_execute_pcm or
                               zafx_run_host_pcm; clips of different lengths go through zafx_execute_center_ragged */
    ZAFX_MASKFILTER = 13,   /* in (B, N) f32 mono and a real mask (B, W/2+1, T) f32 [FT: rows at zafx_plan_row_pitch, the array a
                               ZAFX_SPECTRUM_MAGNITUDE STFT plan of the same layout and row_align writes] or (B, T, W/2+1) [TF], T = ceil(N / H) + 1
                               (zafx_plan_mask_dims) -> out (B, N) f32: y = istft(concat(m, m[-2:0:-1]) * stft(x))[0:N], zaf.py:185-195 with the
                               caller's mask.  Through zafx_execute_masked only.  float32 only, window_length 256 / 512 / 1024 / 2048,
                               step_length = window_length / 2 (as the center kinds).  Two neighbouring frames of one clip share a complex
                               transform: rounding error and a non-finite value of frame 2j+1 reach frame 2j (H samples further than in the
                               reference), never another clip.  n_in = N samples; zafx_plan_out_dims: dims[0] = samples written per clip, dims[1] = 1 */
    ZAFX_MASKFILTER_REST = 14 /* as ZAFX_MASKFILTER -> out (B, 2, N): block 0 of a clip the filtered clip, bit-identical to ZAFX_MASKFILTER's,
                               block 1 the rest = input - block 0 in float32 (the filter of mask 1 - m) */
};

enum zafx_layout {
    ZAFX_LAYOUT_FT = 0, /* reference memory order: frequency-major, time minor (zaf.py:128) */
    ZAFX_LAYOUT_TF = 1  /* frame-major: each frame's bins contiguous                        */
};

enum zafx_spectrum {      /* STFT output / ISTFT input rows                             */
    ZAFX_SPECTRUM_TWO_SIDED = 0, /* W rows, as np.fft.fft returns them (zaf.py:139) -- the reference contract  */
    ZAFX_SPECTRUM_ONE_SIDED = 1, /* rows 0..W/2 only (what every example keeps, zaf.py:83); the ISTFT completes
                                    X[W-k] = conj X[k], i.e. equals istft of the two-sided spectrum of a real signal */
    ZAFX_SPECTRUM_MAGNITUDE = 2, /* STFT only: |X[k]|, k = 0..W/2, real (float32 / float64) -- the spectrogram the
                                    examples compute, np.absolute(audio_stft[0:W/2+1]) (zaf.py:83)                   */
    ZAFX_SPECTRUM_POWER = 3      /* STFT only: |X[k]|^2, k = 0..W/2, real                                          */
};

enum zafx_precision {     /* device arithmetic and array types                          */
    ZAFX_PRECISION_F32 = 0, /* float32 / complex64 arrays and arithmetic (every kind)                        */
    ZAFX_PRECISION_F64 = 1  /* every kind but ZAFX_LINEAR: float64 / complex128 arrays AND constants (window float64[W],
                               mel filterbank / DCT rows float64, CQT values complex128); the reference's own dtype
                               (zaf.py:128, :139), results within 1e-12 of it (mfcc 1e-10); any power-of-two window.
                               window_length 2048 in the reference layout (CQT: fft_length 32768, kernel columns in the one-sided
                               bins 1..8191) runs on tiled kernels of its own -- k_stft_ft8_f64, k_istft_ft8_f64,
                               k_mdct_ft16_f64, k_imdct_ft16_f64 (round 5), k_mel_ft8_f64, k_cqt_ft_f64 (round 6): 2-3 x
                               behind the float32 kernels --, every other geometry one workgroup per frame (5-10 x)   */
};

enum zafx_constant {
    ZAFX_CONST_WINDOW = 1,      /* float32[W]                                   (window_function)  */
    ZAFX_CONST_MEL_FB = 2,      /* float32[n_filters * W/2], dense row-major    (FB.toarray())     */
    ZAFX_CONST_DCT = 3,         /* float32[n_coefs * n_filters], row-major      (DCT-II rows 1..)  */
    ZAFX_CONST_CQT_INDPTR = 4,  /* int32[n_bins + 1]                            (CSR of cqt_kernel) */
    ZAFX_CONST_CQT_INDICES = 5, /* int32[nnz], 0 <= col < fft_length                                */
    ZAFX_CONST_CQT_VALUES = 6,  /* complex64[nnz]                                                   */
    ZAFX_CONST_MATRIX = 7       /* float32[n_filters * window_length], row-major   (ZAFX_LINEAR)      */
};

typedef struct zafx_params {
    int32_t struct_size;       /* = sizeof(zafx_params)                                         */
    int32_t window_length;     /* W, power of two, 64..8192 (STFT family, MDCT family, float32 MEL / MFCC), or --
                                  ZAFX_STFT / ZAFX_ISTFT / ZAFX_MEL / ZAFX_MFCC / ZAFX_MDCT / ZAFX_IMDCT -- any other length 33..8192 (MDCT family: even):
                                  those run as float32 Bluestein convolutions (np.fft takes any length, so does the reference).
                                  With ZAFX_PRECISION_F64 any length 2..2048 (MDCT family: even, 4..2048), every kind            */
    int32_t step_length;       /* hop H >= 1 (STFT/MEL/MFCC: any, also above W as zaf.stft allows; ISTFT: H <= W and
                                  any: above ceil(W/H) = 16 frames (8 at W = 4096, 4 at 8192) the float32 frames +
                                  gather overlap-add form runs instead of the tiled kernel); CQT: frame step        */
    int32_t layout;            /* enum zafx_layout of the 2-D (frequency x time) side           */
    int32_t n_filters;         /* MEL / MFCC: 1..576 (above 256: spectrum kernel + k_melfb; ZAFX_PRECISION_F64: 1..W/2) */
    int32_t n_coefs;           /* MFCC                                                          */
    int32_t fft_length;        /* CQT / CHROMA: power of two, 512..32768; 65536 when the kernel matrix touches the one-sided
                                  bins 1..8191 only (low-frequency kernels); ..131072 with ZAFX_PRECISION_F64 */
    int32_t n_bins;            /* CQT / CHROMA                                                  */
    int32_t octave_resolution; /* CHROMA                                                        */
    int32_t spectrum;          /* enum zafx_spectrum (STFT / ISTFT); 0 = reference contract     */
    int32_t precision;         /* enum zafx_precision (STFT / ISTFT); 0 = float32               */
    int32_t row_align;         /* ZAFX_LAYOUT_FT only: every row of the 2-D (F, T) array starts at a multiple of this many
                                  elements, i.e. the row pitch is T rounded up (zafx_plan_row_pitch).  0 / 1 = compact,
                                  the reference's own memory order.  16 (complex64) / 32 (float32) put every row on a
                                  128-byte line whatever T is -- the reference-layout STFT store runs at full rate only
                                  then (T = 433 compact: 2.1x slower than T = 432; padded: the same).  Power of two
                                  <= 1024.  The padding elements are never written (forward) nor used (inverse).     */
    int32_t transform_type;    /* ZAFX_DCT: 1, 2, 3 or 4 (dct_type / dst_type of zaf.py:703, :842)                    */
    int32_t transform_sine;    /* ZAFX_DCT: 0 = zaf.dct, 1 = zaf.dst                                                */
    int32_t with_mel;          /* ZAFX_MFCC, float32, window_length 2048, <= 128 filters, <= 32 coefficients: 1 = the melspectrogram of the SAME
                                  transforms rides along (zaf.melspectrogram and zaf.mfcc both start with zaf.stft, zaf.py:369 / :436; BASELINE
                                  config 3 in one pass: k_mel2 MODE 4).  Output = n_filters + n_coefs rows per clip: rows 0 .. n_filters - 1 the
                                  melspectrogram, the rest the MFCCs -- both bit-identical to the single-output plans' results           */
    int32_t reserved[1];
} zafx_params;

/* ---- library / device ------------------------------------------------------------ */
int zafx_version(void);
const char* zafx_last_error(void);
int zafx_device_count(int* count);
int zafx_device_name(int device, char* buf, size_t buflen);

/* ---- device memory (synchronous helpers; caller owns the allocations) -------------- */
#define ZAFX_ERROR_OUT_OF_MEMORY 2 /* zafx_alloc: the device has no room (= hipErrorOutOfMemory); other codes are other faults */
/* Arrays of 1 GiB and more are assembled from separate physical allocations of ZAFX_ALLOC_CHUNK_MB (default 64) MiB mapped back to back into one range
 * (HIP's virtual-memory API; 0 = plain hipMalloc): where a multi-GB array lies in physical memory moves the kernels that write it by up to 12 %, and on most
 * boxes the chunked form lands where hipMalloc's first allocation does not.  Pointers from zafx_alloc go back to zafx_free, not to hipFree. */
int zafx_alloc(int device, void** dptr, size_t bytes);
int zafx_free(int device, void* dptr);
/* The fastest of `n_candidates` allocations of `bytes` for the OUTPUT of `plan` (no reference counterpart).  Where a
 * multi-GB array lands in physical memory changes the rate of the kernels that write it with a row stride -- the reference layout's
 * (W, T) spectra of zaf.py:139: the same STFT runs in 1.51 ms into one 7.25 GB allocation and in 1.70 ms into another of the same
 * process -- and the address is not the caller's to choose, so a long-lived output buffer is picked by trial: all candidates are
 * allocated (held at once: a freed one would come straight back), zafx_execute(plan, d_in, candidate, n_clips, n_in) is timed on each
 * (one untimed launch, then `reps`; HIP events on the plan's stream), the best stays in *dptr, the others are freed.
 * probe_ms: NULL or n_candidates floats (the time per launch of each candidate).  bytes must hold the plan's output for (n_clips,
 * n_in).  Fewer candidates than asked are tried when the device runs out of memory (at least one).  The C twin of the Python
 * layer's DeviceBuffer.placed. */
int zafx_alloc_placed(zafx_plan* plan, void** dptr, size_t bytes, const void* d_in, int64_t n_clips, int64_t n_in, int n_candidates, int reps,
                      float* probe_ms);
/* Plain fills and copies.  All four return when the bytes are in place -- zafx_memset and zafx_d2d wait for the device, which hipMemset and a
 * device-to-device hipMemcpy alone do not --, so a plan's stream, which does not wait for the null stream, sees them whatever is enqueued next. */
int zafx_memset(int device, void* dptr, int value, size_t bytes);
int zafx_h2d(int device, void* dst, const void* src, size_t bytes);
int zafx_d2h(int device, void* dst, const void* src, size_t bytes);
int zafx_d2d(int device, void* dst, const void* src, size_t bytes);

/* Page-locked host memory for the transfers above: pageable NumPy buffers move at ~25 GB/s (and fault on first
 * touch), pinned ones at the PCIe rate (~56 GB/s measured).  Free with zafx_host_free. */
int zafx_host_alloc(void** hptr, size_t bytes);
int zafx_host_free(void* hptr);

/* ---- plans -------------------------------------------------------------------------- */
/* Environment read when a plan is created:
 *   ZAFX_COMPUTE_UNITS=n   (n >= 1) the plan sizes every persistent grid, every cut of clips into carry segments and every slot count of a
 *                          ragged launch for min(n, the device's count) compute units instead of the device's count: to leave compute units
 *                          to other work on the same device, and to test the kernels on the grids a smaller device would give them.  Unset,
 *                          empty, 0 or not a whole number: the device's count.  The results do not depend on it, bit for bit.
 *   ZAFX_STFT_DYNAMIC=0    k_stft_ft16 deals its tiles out up front instead of claiming them at run time. */
int zafx_plan_create(zafx_plan** plan, int device, int kind, const zafx_params* params);
int zafx_plan_destroy(zafx_plan* plan);
/* The number of device and page-locked allocations that plans of this process own right now (*count): tables, constants and the grow-only
 * staging buffers of the execute calls -- every one is released by zafx_plan_destroy, so the count is back at its earlier value once a plan
 * is gone, and a zafx_plan_create that fails leaves it as it was.  The arrays of zafx_alloc / zafx_host_alloc are the caller's and are not
 * counted.  Needs no device. */
int zafx_plan_live_allocations(int64_t* count);
/* Upload one constant (copied; the host buffer may be released on return).
 * The call may be repeated between calls on the plan, at any time: it waits for the plan's stream (work already enqueued finishes with the
 * constants it was enqueued under), replaces the constant and rebuilds everything derived from it.  Every later execute -- the ragged and the
 * PCM entry points included -- gives, bit for bit, what a plan created with the constants now in place gives, on the kernel that plan runs (zafx_plan_kernel_name follows the
 * last upload, zafx_plan_last_kernel_name the next execute).  An upload the call refuses (a wrong size, an id the kind does not take, a CQT column
 * outside 0 .. fft_length - 1) leaves the plan unchanged.  The three arrays of a CQT kernel arrive one by one, so the lengths of
 * ZAFX_CONST_CQT_INDICES and _VALUES are checked against each other where they are used: zafx_execute refuses a plan whose CSR arrays
 * disagree and writes nothing (tests/test_gpu_constants.py).  An upload that was accepted and then fails on the device (no memory for a
 * derived table, say: the HIP error is returned) leaves that constant unset or half rebuilt: upload it again before the next execute. */
int zafx_plan_set_constant(zafx_plan* plan, int which, const void* host, size_t bytes);
/* Output geometry for `n_in` (samples per clip for forward kinds, frames T for inverse
 * kinds): dims[0] = rows F (or samples L), dims[1] = frames T (or 1). */
int zafx_plan_out_dims(const zafx_plan* plan, int64_t n_in, int64_t dims[2]);
/* Elements between the starts of consecutive rows of the plan's 2-D array for `n_in` (as above): T for compact
 * plans, T rounded up to params.row_align otherwise; the array then holds clips x F x pitch elements.  For
 * ZAFX_LAYOUT_TF and ZAFX_LINEAR plans this is the (contiguous) row length itself. */
int zafx_plan_row_pitch(const zafx_plan* plan, int64_t n_in, int64_t* pitch);
/* Enqueue the transform of n_clips clips on the plan's stream (asynchronous).
 *
 * The length of ONE clip.  Several kernels address a clip through one buffer descriptor with 32-bit byte offsets; the launchers take them
 * only below the lengths listed here and run another kernel -- same result, same bounds, lower rate -- from there on, so no length
 * changes what is computed (float32, ZAFX_LAYOUT_FT; tests/test_gpu_long_clips.py runs one clip on either side of each):
 *   ZAFX_STFT, |X| and |X|^2 at window 2048   k_mel2 for n_in < 2^29 samples, k_stft_ft16 from there on
 *   ZAFX_STFT, complex, rows off the line grid   the buffer-load form of k_stft_ft16c / k_stft_ft16bc while T x hop < 2^29, its pointer form /
 *                                             the one-workgroup-per-tile kernel above; window 4096 and 8192: (T + 16) x hop < 2^29 / 2^28
 *   ZAFX_ISTFT                                the tiled kernels while window x row pitch x 8 < 2^31 bytes -- window rows counted for a one-sided
 *                                             spectrum too: 131072 frames at window 2048, 65536 at 4096, 32768 at 8192 --, k_istft above
 *   ZAFX_MDCT                                 16-byte loads for n_in < 2^28 (window 512 ... 2048: k_mdct_ft32's 4-byte form above; window 4096: the two-band
 *                                             kernels k_mdct_ft32b / k_mdct_ft32bc below, k_mdct above); window 8192: k_mdct_ft32q while (T + 33) x 4096 < 2^28,
 *                                             k_mdct above
 *   ZAFX_IMDCT                                16-byte gathers while window / 2 x row pitch x 4 < 2^32 bytes; window 8192: k_imdct_q while
 *                                             4096 x row pitch x 4 < 2^31, k_imdct above
 *   ZAFX_MEL / ZAFX_MFCC                      buffer loads for n_in < 2^29; window 4096: k_mel_ft16b while (T + 16) x hop < 2^29, the
 *                                             spectrum kernel + k_melfb above
 * Two kinds REFUSE long clips: the call returns an error (zafx_last_error names the limit), enqueues nothing and writes nothing.
 *   ZAFX_CQT / ZAFX_CHROMA (float32)          n_in >= 2^29 samples (3.4 h at 44.1 kHz): cut the signal
 *   ZAFX_CENTER / ZAFX_CENTER_SIDES           n_in >= 2^28 sample frames (1.7 h at 44.1 kHz)
 *   ZAFX_MASKFILTER / ZAFX_MASKFILTER_REST    n_in >= 2^28 samples (zafx_execute_masked; zafx_execute_masked_ragged, zafx_execute_masked_stems_ragged: any clip of the batch)
 *                                             complex masks: n_in >= 2^27 samples (zafx_execute_masked_complex; zafx_execute_masked_complex_ragged: any clip of the batch)
 *                                             stereo clips: n_in >= 2^28 sample frames, 2^27 with a mask per channel (zafx_execute_masked_stereo;
 *                                             zafx_execute_masked_stereo_ragged: any clip of the batch)
 * zafx_execute_pcm reads int16 in the kernels' own loads below the same lengths (n_frames < 2^29; the MDCT: < 2^28) and converts first above them.
 * Not run at its bound by any test yet: the two-sided complex STFT at window 8192 (k_stft_ft16q takes whole-line rows only; its |X| kind is run).
 * The ragged and PCM entry points state their own per-clip limits below. */
int zafx_execute(zafx_plan* plan, const void* d_in, void* d_out, int64_t n_clips, int64_t n_in);
/* The mask filter of n_clips mono clips of n_in samples, enqueued on the plan's stream (asynchronous; ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST
 * plans only, which zafx_execute, zafx_execute_ragged, zafx_execute_pcm and zafx_run_host* refuse; every other kind is refused here; last
 * kernel "k_maskfilter").  d_mask: one real float32 mask per clip, zafx_plan_mask_dims rows x frames: in ZAFX_LAYOUT_FT (B, rows, pitch) with
 * pitch = zafx_plan_row_pitch(plan, n_in) -- frames for a compact plan, frames rounded up to params.row_align otherwise; the padding and
 * anything from column `frames` on is never read --, in ZAFX_LAYOUT_TF (B, frames, rows) compact, which reads whole lines and is the
 * faster of the two.  The three arrays need 4-byte alignment only.  Nothing is read in front of sample 0 or from sample
 * n_in on, nothing is written at or beyond n_in; no clip's result depends on another clip's samples or mask, and a clip has the same
 * bits alone, anywhere in a batch and under any ZAFX_COMPUTE_UNITS.  A mask of zeros gives exact zeros, and so does silence under any
 * finite mask.  Rejected with a message, nothing enqueued or written: a null plan or pointer, negative sizes, another kind, a window
 * that is not set or whose sum(window[0:W:H]) is zero, clips of 2^28 samples and more. */
int zafx_execute_masked(zafx_plan* plan, const void* d_in, const void* d_mask, void* d_out, int64_t n_clips, int64_t n_in);
/* The mask of one clip of n_in samples under a ZAFX_MASKFILTER / _REST plan: dims[0] = rows W/2 + 1, dims[1] = frames T = ceil(n_in / H) + 1,
 * the frame count of zaf.stft (zaf.py:99-109).  zafx_plan_row_pitch(plan, n_in) gives the elements between its rows. */
int zafx_plan_mask_dims(const zafx_plan* plan, int64_t n_in, int64_t dims[2]);
/* Mask placement of a ragged mask-filter batch: the mask of clip i is zafx_plan_mask_dims(plan, lengths[i]) -- in ZAFX_LAYOUT_FT rows x
 * zafx_plan_row_pitch(plan, lengths[i]), in ZAFX_LAYOUT_TF frames x rows compact -- at element mask_offsets[i] of the mask array; the masks
 * lie back to back and mask_offsets[n_clips] = total elements.  A length of 0 has the one-frame mask zafx_plan_mask_dims gives; it is never
 * read.  This is the layout zafx_plan_ragged_layout gives a one-sided ZAFX_SPECTRUM_MAGNITUDE ZAFX_STFT plan of the same window, layout and
 * row_align, so the |X| a ragged STFT writes can be turned into masks where it lies. */
int zafx_plan_mask_ragged_layout(const zafx_plan* plan, const int64_t* lengths, int64_t n_clips, int64_t* mask_offsets);
/* The mask filter of n_clips mono clips of different lengths in ONE launch (ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans only; last
 * kernel "k_maskfilter_ragged"), enqueued on the plan's stream (asynchronous).  Offsets and lengths count float32 elements: clip i is
 * lengths[i] samples at element in_offsets[i] of d_in -- clips may lie back to back, each is padded with zeros of its own --, its mask
 * (shape and pitch as zafx_plan_mask_ragged_layout describes) starts at element mask_offsets[i] of d_mask -- any placement will do; the pad
 * columns of a row and anything behind a mask's last frame are never read --, and its filtered samples go to element out_offsets[i] of
 * d_out; under ZAFX_MASKFILTER_REST the rest follows directly behind, at out_offsets[i] + lengths[i] (the (2, N_i) block of the
 * equal-length kind, one per clip).  Every clip's result is bit-identical to zafx_execute_masked on that clip and mask alone.  A clip of
 * length 0 is skipped: nothing of it is read or written.  The four host arrays are copied before return.  The arrays need 4-byte alignment
 * only.  Rejected with a message, nothing enqueued or written: a null plan, pointer or host array, n_clips < 0, another kind, negative
 * lengths or offsets (with the clip's index), a clip of 2^28 samples or more, a window that is not set or whose sum(window[0:W:H]) is
 * zero.  NOT checked: that the output blocks do not overlap -- placing them is the caller's business. */
int zafx_execute_masked_ragged(zafx_plan* plan, const void* d_in, const int64_t* in_offsets, const int64_t* lengths, const void* d_mask,
                               const int64_t* mask_offsets, void* d_out, const int64_t* out_offsets, int64_t n_clips);
/* The mask filter under a COMPLEX mask: zafx_execute_masked with one complex64 mask M per clip (interleaved re, im), enqueued on the plan's
 * stream (asynchronous; ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans created with ZAFX_LAYOUT_TF only; last kernel "k_maskfilter_complex"):
 *     y = istft(concat(M, conj(M[-2:0:-1])) * stft(x, w, H), w, H)[0:n_in]        (zaf.py:185-195; istft keeps the real part, zaf.py:223)
 * -- phase-aware masks, any per-bin linear filter.  d_in (B, n_in) float32; d_mask (B, frames, rows) complex64 compact, rows x frames =
 * zafx_plan_mask_dims counted in complex elements; d_out (B, n_in) float32, under ZAFX_MASKFILTER_REST (B, 2, n_in) with block 1 =
 * input - block 0 in float32, bit-equal to the subtraction of the block 0 that was written.  All three arrays need 4-byte alignment only,
 * the complex mask included.  The imaginary parts of mask rows 0 and W/2 have no effect: those bins are their own mirror, the kernel
 * discards the values (it does not multiply them by zero), and they may hold anything, NaN included.  CONTRACT, as zafx_execute_masked's:
 * two neighbouring frames of one clip share a transform, so rounding and non-finite values couple frames 2j and 2j+1 of one clip and never
 * reach another clip; nothing is read in front of a clip's sample 0, from its sample n_in on or behind a mask's last frame, nothing is
 * written at or beyond n_in; a clip has the same bits alone, anywhere in a batch, however it is cut and under any ZAFX_COMPUTE_UNITS; a mask
 * of zeros gives exact zeros, and so does silence under any finite mask.  NOT promised: the bits of zafx_execute_masked where every
 * imaginary part is zero -- the library is built with -ffp-contract=fast and the two pair functions contract differently; the results
 * agree within the accuracy of either.  Rejected with a message, nothing enqueued or written: a null plan or pointer, negative sizes,
 * another kind, a plan in ZAFX_LAYOUT_FT (the mask stage in LDS would double; the message names ZAFX_LAYOUT_TF), a window that is not set
 * or whose sum(window[0:W:H]) is zero, clips of 2^27 samples and more (the mask -- 8 bytes a bin -- lies behind signed 32-bit byte
 * offsets).  The other entry points on the same plan are not affected. */
int zafx_execute_masked_complex(zafx_plan* plan, const void* d_in, const void* d_mask, void* d_out, int64_t n_clips, int64_t n_in);
/* zafx_execute_masked_complex for n_clips mono clips of different lengths in ONE launch (ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans
 * created with ZAFX_LAYOUT_TF only; last kernel "k_maskfilter_complex_ragged").  in_offsets, lengths and out_offsets count float32
 * elements as in zafx_execute_masked_ragged, and the output blocks are placed as there (the rest directly behind, at out_offsets[i] +
 * lengths[i]); mask_offsets counts COMPLEX64 elements: the mask of clip i, (T_i, W/2 + 1) compact, starts at complex element
 * mask_offsets[i] of d_mask.  Any placement will do; zafx_plan_mask_ragged_layout on the plan gives the compact one as it stands (rows x
 * frames elements per clip) -- which is also the layout zafx_plan_ragged_layout gives a one-sided complex ZAFX_LAYOUT_TF STFT plan, so the
 * spectra a ragged STFT writes can be turned into masks where they lie.  The arrays need 4-byte alignment only.  CONTRACT: clip i's block is
 * bit-identical to zafx_execute_masked_complex on that clip and mask alone, whatever the batch and however the clip is cut; no clip sees
 * another's samples or mask; the imaginary parts of mask rows 0 and W/2 have no effect, as above.  A clip of length 0 is skipped, an empty
 * batch is fine.  Rejected with a message, nothing enqueued or written: a null plan, pointer or host array, a negative count, another kind,
 * a plan in ZAFX_LAYOUT_FT, negative lengths or offsets (with the clip's index), a clip of 2^27 samples or more (with its index; decided on
 * `lengths` before anything is read), a window that is not set or whose COLA sum is zero.  ZAFX_MASKFILTER_UNITS_PER_SLOT in the
 * environment applies as it does to zafx_execute_masked_ragged (measurements only). */
int zafx_execute_masked_complex_ragged(zafx_plan* plan, const void* d_in, const int64_t* in_offsets, const int64_t* lengths, const void* d_mask,
                                       const int64_t* mask_offsets, void* d_out, const int64_t* out_offsets, int64_t n_clips);
/* Stems: n_stems masks per clip over ONE forward transform, n_stems inverse transforms, in one launch (ZAFX_MASKFILTER and
 * ZAFX_MASKFILTER_REST plans created with ZAFX_LAYOUT_TF only; last kernel "k_maskfilter_stems", for n_stems == 1 too), enqueued on the
 * plan's stream (asynchronous).  d_in (B, n_in) float32 samples; d_mask (B, n_stems, frames, rows) float32 compact, frames x rows =
 * zafx_plan_mask_dims of ZAFX_LAYOUT_TF, the masks of a clip back to back; d_out (B, n_stems, n_in) float32: block s of a clip is that clip
 * filtered with its mask s.  ZAFX_MASKFILTER_REST: d_out (B, n_stems + 1, n_in), and block n_stems of a clip holds the rest
 * ((x - y_0) - y_1) - ... - y_{n_stems-1}, float32, subtracted in that order from the samples as read.  Stem s of every clip is
 * bit-identical to zafx_execute_masked on that clip with mask s alone under a ZAFX_LAYOUT_TF plan -- whatever n_stems and the other stems'
 * masks, wherever the clip lies in the batch, under any ZAFX_COMPUTE_UNITS --, so a mask of zeros gives exact zeros in its stem, silence
 * gives exact zeros everywhere, and a non-finite value stays within its own clip.  The three arrays need 4-byte alignment only.  Nothing
 * is read in front of a clip's sample 0 or from its sample n_in on, nothing behind a mask's last frame, and nothing is written at or
 * beyond sample n_in of a block.  Rejected with a message, nothing enqueued or written: a null plan or pointer, negative sizes, another
 * kind, a plan in ZAFX_LAYOUT_FT (the message names ZAFX_LAYOUT_TF), n_stems outside 1 .. ZAFX_MASKFILTER_MAX_STEMS, a window that is not
 * set or whose sum(window[0:W:H]) is zero, clips of 2^28 samples and more.  zafx_execute_masked and zafx_execute_masked_ragged on the same
 * plan are not affected. */
#define ZAFX_MASKFILTER_MAX_STEMS 8
int zafx_execute_masked_stems(zafx_plan* plan, const void* d_in, const void* d_mask, void* d_out, int64_t n_clips, int64_t n_in,
                              int32_t n_stems);
/* Placement of a ragged stems batch (ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans of ZAFX_LAYOUT_TF, n_stems in 1 ..
 * ZAFX_MASKFILTER_MAX_STEMS), in float32 elements, both arrays of n_clips + 1 entries: the n_stems masks of clip i lie back to back as
 * (n_stems, T_i, W/2 + 1), T_i = zafx_plan_mask_dims(plan, lengths[i])[1], at element mask_offsets[i] of the mask array, the clips back to
 * back -- n_stems x what zafx_plan_mask_ragged_layout gives --; its output block is (n_stems, lengths[i]), under ZAFX_MASKFILTER_REST
 * (n_stems + 1, lengths[i]), at element out_offsets[i], the blocks back to back.  Entry n_clips of either array is the total.  A clip of
 * length 0 has T = 1 (its masks are never read) and an empty output block. */
int zafx_plan_stems_ragged_layout(const zafx_plan* plan, const int64_t* lengths, int64_t n_clips, int32_t n_stems, int64_t* mask_offsets,
                                  int64_t* out_offsets);
/* Ragged stems: zafx_execute_masked_stems for n_clips mono clips of different lengths in ONE launch (ZAFX_MASKFILTER and
 * ZAFX_MASKFILTER_REST plans created with ZAFX_LAYOUT_TF only; last kernel "k_maskfilter_stems_ragged"), enqueued on the plan's stream
 * (asynchronous).  n_stems is one value for the batch.  Offsets and lengths count float32 elements: clip i is lengths[i] samples at element
 * in_offsets[i] of d_in; its n_stems masks, each (T_i, W/2 + 1) compact, lie back to back from element mask_offsets[i] of d_mask; its
 * output block -- (n_stems, lengths[i]), under ZAFX_MASKFILTER_REST (n_stems + 1, lengths[i]) with the rest
 * ((x - y_0) - y_1) - ... - y_{n_stems-1} in its last row -- starts at element out_offsets[i] of d_out.  Any placement of clips, masks and
 * output blocks will do (zafx_plan_stems_ragged_layout gives the compact one): clips and masks may lie back to back -- every clip is
 * padded with zeros of its own, and nothing behind a stem's last frame is read for that stem --, and nothing is written outside the output
 * blocks.  The arrays need 4-byte alignment only.  CONTRACT: clip i's block is bit-identical to zafx_execute_masked_stems on that clip and
 * its n_stems masks alone, so stem s is bit-identical to zafx_execute_masked with mask s alone -- whatever the batch, the clip's place in
 * it, the cut into units and ZAFX_COMPUTE_UNITS.  A clip of length 0 is skipped: nothing of it is read or written; an empty batch is
 * fine.  The four host arrays are copied before return.  Rejected with a message, nothing enqueued or written: a null plan, pointer or host
 * array, n_clips < 0, another kind, a plan in ZAFX_LAYOUT_FT (the message names ZAFX_LAYOUT_TF), n_stems outside 1 ..
 * ZAFX_MASKFILTER_MAX_STEMS, negative lengths or offsets (with the clip's index), a clip of 2^28 samples or more (with its index; decided
 * on `lengths` before anything is read), a window that is not set or whose sum(window[0:W:H]) is zero.  NOT checked: that the output
 * blocks do not overlap.  Every other entry point on the same plan is not affected.  ZAFX_MASKFILTER_UNITS_PER_SLOT in the environment
 * applies as it does to zafx_execute_masked_ragged (measurements only). */
int zafx_execute_masked_stems_ragged(zafx_plan* plan, const void* d_in, const int64_t* in_offsets, const int64_t* lengths, const void* d_mask,
                                     const int64_t* mask_offsets, void* d_out, const int64_t* out_offsets, int64_t n_clips, int32_t n_stems);
/* The mask filter for INTERLEAVED STEREO clips under masks of the caller's, enqueued on the plan's stream (asynchronous; ZAFX_MASKFILTER and
 * ZAFX_MASKFILTER_REST plans created with ZAFX_LAYOUT_TF only; last kernel "k_maskfilter_stereo"):
 *     y[:, c] = istft(concat(m_c, m_c[-2:0:-1]) * stft(x[:, c], w, H), w, H)[0:n_in],  c = L, R        (zaf.py:176-198 with the caller's masks)
 * mask_channels == 1: one mask for both channels, m_L = m_R; mask_channels == 2: one per channel.  d_in (B, n_in, 2) float32, n_in counted in
 * sample frames; d_mask float32 compact, (B, frames, rows) for mask_channels == 1 and (B, frames, 2, rows) for 2 -- a frame's L row lies
 * directly in front of its R row --, rows x frames = zafx_plan_mask_dims; d_out (B, n_in, 2), under ZAFX_MASKFILTER_REST (B, 2, n_in, 2) with
 * block 1 = input - block 0 in float32, bit-equal to the subtraction of the block 0 that was written (the layout of ZAFX_CENTER_SIDES).  The
 * arrays need 4-byte alignment only.  CONTRACT: the two channels of a frame share one transform, so rounding (a quiet channel beside a loud
 * one carries about eps32 of the loud level) and a non-finite sample or mask value of one channel reach the other channel of the same frames
 * -- output blocks j - 1 and j for frame j -- and never another frame pair or another clip; nothing is read in front of a clip's sample
 * frame 0, from its sample frame n_in on or behind a mask's last frame, nothing is written at or beyond n_in; a clip has the same bits alone,
 * anywhere in a batch, however it is cut and under any ZAFX_COMPUTE_UNITS; a mask of zeros gives exact zeros, and so does silence on both
 * channels under any finite mask.  NOT promised: that two equal per-channel masks give the bits of the shared form (that one scales the
 * packed spectrum without splitting it), nor that a channel has the bits zafx_execute_masked gives it as a mono clip (the packing differs);
 * all agree within the accuracy of either.  Rejected with a message, nothing enqueued or written: a null plan or pointer, negative sizes,
 * another kind, a plan in ZAFX_LAYOUT_FT (the message names ZAFX_LAYOUT_TF), mask_channels outside {1, 2}, a window that is not set or whose
 * sum(window[0:W:H]) is zero, clips of 2^28 sample frames and more (8 bytes a sample frame behind one descriptor) -- 2^27 with
 * mask_channels == 2 (two masks per frame are 8 bytes a bin, the complex kind's arithmetic).  The other entry points on the same plan are
 * not affected. */
int zafx_execute_masked_stereo(zafx_plan* plan, const void* d_in, const void* d_mask, void* d_out, int64_t n_clips, int64_t n_in,
                               int32_t mask_channels);
/* Placement of a ragged stereo batch (ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans of ZAFX_LAYOUT_TF, mask_channels 1 or 2), both arrays
 * of n_clips + 1 entries: the masks of clip i, (T_i, mask_channels, W/2 + 1), start at float32 element mask_offsets[i] of the mask array, the
 * clips back to back -- mask_channels x what zafx_plan_mask_ragged_layout gives --; its output block of lengths[i] sample frames, under
 * ZAFX_MASKFILTER_REST two of them, starts at SAMPLE FRAME out_offsets[i], the blocks back to back.  Entry n_clips of either array is the
 * total.  A clip of length 0 has T = 1 (its masks are never read) and an empty output block. */
int zafx_plan_stereo_ragged_layout(const zafx_plan* plan, const int64_t* lengths, int64_t n_clips, int32_t mask_channels, int64_t* mask_offsets,
                                   int64_t* out_offsets);
/* zafx_execute_masked_stereo for n_clips stereo clips of different lengths in ONE launch (ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans
 * created with ZAFX_LAYOUT_TF only; last kernel "k_maskfilter_stereo_ragged").  in_offsets, lengths and out_offsets count SAMPLE FRAMES, as in
 * zafx_execute_center_ragged: clip i is lengths[i] sample frames at sample frame in_offsets[i] of d_in, its output block starts at sample
 * frame out_offsets[i] of d_out and, under ZAFX_MASKFILTER_REST, the rest follows at out_offsets[i] + lengths[i].  mask_offsets counts float32
 * elements: the masks of clip i, (T_i, mask_channels, W/2 + 1) compact, start at element mask_offsets[i] of d_mask.  Any placement will do
 * (zafx_plan_stereo_ragged_layout gives the compact one); the arrays need 4-byte alignment only.  CONTRACT: clip i's block is bit-identical
 * to zafx_execute_masked_stereo on that clip and its masks alone, whatever the batch, its cut and ZAFX_COMPUTE_UNITS; no clip sees another's
 * samples or masks.  A clip of length 0 is skipped, an empty batch is fine.  The four host arrays are copied before return.  Rejected with a
 * message, nothing enqueued or written: a null plan, pointer or host array, a negative count, another kind, a plan in ZAFX_LAYOUT_FT,
 * mask_channels outside {1, 2}, negative lengths or offsets (with the clip's index), a clip of 2^28 sample frames or more, 2^27 with
 * mask_channels == 2 (with its index; decided on `lengths` before anything is read), a window that is not set or whose COLA sum is zero.
 * NOT checked: that the output blocks do not overlap.  ZAFX_CENTER_UNITS_PER_SLOT in the environment applies as it does to
 * zafx_execute_center_ragged (measurements only). */
int zafx_execute_masked_stereo_ragged(zafx_plan* plan, const void* d_in, const int64_t* in_offsets, const int64_t* lengths, const void* d_mask,
                                      const int64_t* mask_offsets, void* d_out, const int64_t* out_offsets, int64_t n_clips, int32_t mask_channels);
/* The mask filter on 16-BIT PCM, enqueued on the plan's stream (asynchronous; ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans created with
 * ZAFX_LAYOUT_TF only): the kernels read int16 samples in their own loads and, with out_sample_bytes == 2, write int16 samples in their own
 * stores -- no float32 staging array on either side.  n_channels == 1: mono clips, d_pcm (B, n_frames) int16, mask_channels must be 1, d_mask
 * as zafx_execute_masked takes it in ZAFX_LAYOUT_TF, (B, frames, rows) float32 (last kernel "k_maskfilter_pcm").  n_channels == 2:
 * interleaved stereo, d_pcm (B, n_frames, 2) int16, mask_channels 1 or 2 and d_mask as zafx_execute_masked_stereo takes them (last kernel
 * "k_maskfilter_stereo_pcm").  d_out has the shape of the float entry point's output -- with rest (B, 2, n_frames[, 2]) -- in float32
 * (out_sample_bytes == 4) or int16 (2).  ARITHMETIC: sample s enters as s / 32768 (zaf.py:1202), exact in float32.
 *   out_sample_bytes == 4: the result is BIT-IDENTICAL to zafx_execute_masked / zafx_execute_masked_stereo on the clip normalised that way,
 *     the rest x / 32768 - y included.
 *   out_sample_bytes == 2: q(y) of that float32 result, with t = y * 32768 in float32: NaN -> 0; t >= 32767 (+inf too) -> 32767;
 *     t <= -32768 (-inf too) -> -32768; anything else rint(t), ties to even.  The rest is integer arithmetic on what was written:
 *     rest = clamp(x - q(y), -32768, 32767), so q(y) + rest == x to the bit wherever the rest did not saturate.
 * Everything else is the float entry point's contract: nothing read in front of sample frame 0 or from n_frames on, nothing written at or
 * beyond n_frames, the same bits alone, anywhere in a batch, however cut and under any ZAFX_COMPUTE_UNITS.  Alignment: mono int16 arrays 2
 * bytes; stereo int16 arrays 4 bytes, the sample-frame grid; float32 arrays (the masks, a float32 output) 4 bytes.  Rejected with a message,
 * nothing enqueued or written: a null plan or pointer, negative sizes, another kind, a plan in ZAFX_LAYOUT_FT, n_channels outside {1, 2},
 * mask_channels 2 with one channel or outside {1, 2}, out_sample_bytes outside {2, 4}, an array off its grid, clips at the bound of the
 * float entry point (2^28 sample frames; 2^27 with two masks), a window that is not set or whose sum(window[0:W:H]) is zero.
 * zafx_execute_pcm, zafx_run_host_pcm and zafx_execute_ragged_pcm go on refusing mask-filter plans. */
int zafx_execute_masked_pcm(zafx_plan* plan, const void* d_pcm, const void* d_mask, void* d_out, int64_t n_clips, int64_t n_frames,
                            int32_t n_channels, int32_t mask_channels, int32_t out_sample_bytes /* 2: int16, 4: float32 */);
/* zafx_execute_masked_pcm for n_clips clips of different lengths in ONE launch (last kernel "k_maskfilter_pcm_ragged" /
 * "k_maskfilter_stereo_pcm_ragged").  in_offsets, lengths and out_offsets count SAMPLE FRAMES: clip i is lengths[i] sample frames at sample
 * frame in_offsets[i] of d_pcm, its output block starts at sample frame out_offsets[i] of d_out and, under ZAFX_MASKFILTER_REST, the rest
 * follows at out_offsets[i] + lengths[i].  mask_offsets counts float32 elements, placed as zafx_plan_mask_ragged_layout (n_channels 1) or
 * zafx_plan_stereo_ragged_layout (2) give them, or anywhere else.  CONTRACT: clip i's block is bit-identical to zafx_execute_masked_pcm on
 * that clip and its masks alone.  A clip of length 0 is skipped, an empty batch is fine.  The four host arrays are copied before return.
 * Rejected as zafx_execute_masked_pcm rejects, and: a null host array, negative lengths or offsets (with the clip's index), a clip at the
 * bound (with its index; decided on `lengths` before anything is read).  NOT checked: that the output blocks do not overlap. */
int zafx_execute_masked_pcm_ragged(zafx_plan* plan, const void* d_pcm, const int64_t* in_offsets, const int64_t* lengths, const void* d_mask,
                                   const int64_t* mask_offsets, void* d_out, const int64_t* out_offsets, int64_t n_clips, int32_t n_channels,
                                   int32_t mask_channels, int32_t out_sample_bytes);
int zafx_sync(zafx_plan* plan);
/* Ragged batches: clips of different lengths in one call (forward kinds that take samples: ZAFX_STFT, _MDCT, _MEL, _MFCC
 * with_mel included, _CQT, _CHROMA; float32 and float64).
 * Output placement: clip i of lengths[i] samples gets its block of the output array at element out_offsets[i];
 * out_offsets[n_clips] = total elements.  FT layout: F rows at zafx_plan_row_pitch(plan, lengths[i]); TF: T_i x F compact.
 * T_i is zafx_plan_out_dims(plan, lengths[i])[1] (a length of 0 gives the reference's single all-zero frame).  The blocks lie
 * back to back, so every block starts on a 128-byte line when the plan's rows are whole lines and the array does.
 * ZAFX_CENTER / ZAFX_CENTER_SIDES plans are refused here and by zafx_execute_ragged: their ragged batches have an entry point
 * of their own, zafx_execute_center_ragged below (the output has the input's shape, so there is no layout to ask for). */
int zafx_plan_ragged_layout(const zafx_plan* plan, const int64_t* lengths, int64_t n_clips, int64_t* out_offsets);
/* Enqueue the transform of n_clips clips of different lengths on the plan's stream (asynchronous): clip i is lengths[i]
 * samples at element in_offsets[i] of d_in; its result goes to the block zafx_plan_ragged_layout assigns.  The two host
 * arrays are copied before return.  Negative lengths or offsets and more than 2^31 - 1 sixteen-frame tiles in all are
 * rejected.  Float32 plans in ZAFX_LAYOUT_FT whose every clip has rows of whole 128-byte lines (params.row_align = one line)
 * and a 128-byte aligned d_out run in ONE launch: the STFT at window 256 ... 2048 on k_stft_ft16 (last kernel
 * "k_stft_ft16_ragged"; |X| / |X|^2 at 2048 on k_mel2), mel / mfcc on k_mel2 where zafx_execute runs them there
 * ("k_mel2_ragged"), the MDCT at window 512, 1024 and 2048 on k_mdct_ft32 ("k_mdct_ft32_ragged": 16-byte loads when d_in is
 * 16-byte aligned and every offset and length is a multiple of 4 samples, 4-byte loads for any other offsets and lengths; every
 * clip below 2^28 samples).  ZAFX_RAGGED_MDCT_NATIVE=0 in the environment keeps MDCT batches off that launch: a switch for
 * measurements only (tools/ragged_rates.py times the launch against one execute per clip in one process), read at every call,
 * not part of the interface.
 * Float64 plans (params.precision = ZAFX_PRECISION_F64) in ZAFX_LAYOUT_FT at window_length 2048 (a power of two: no Bluestein
 * part) run in ONE launch under the same conditions on the output -- every clip's rows whole 128-byte lines (row_align 8 for
 * complex128, 16 for float64), d_out 128-byte aligned -- with d_in 16-byte aligned and fewer than 2^31 tiles: ZAFX_STFT with
 * spectrum ZAFX_SPECTRUM_TWO_SIDED or _ONE_SIDED on k_stft_ft8_f64 ("k_stft_ft8_f64_ragged", 8-frame tiles), ZAFX_MDCT on
 * k_mdct_ft16_f64 ("k_mdct_ft16_f64_ragged"), ZAFX_MEL / ZAFX_MFCC on k_mel_ft8_f64 where zafx_execute runs them there (up to
 * 128 filters; "k_mel_ft8_f64_ragged").  Offsets and lengths are free: a frame that lies inside its clip and starts an even
 * number of samples into d_in is read by 16-byte loads, every other frame sample by sample -- a clip at an odd offset throughout.
 * The bits are those of zafx_execute on each clip.  ZAFX_RAGGED_F64_NATIVE=0 in the environment keeps float64 batches off these
 * launches: for measurements only, read at every call, not part of the interface, as ZAFX_RAGGED_MDCT_NATIVE above and
 * ZAFX_RAGGED_IMDCT_NATIVE, ZAFX_RAGGED_ISTFT_NATIVE and ZAFX_RAGGED_PCM_NATIVE below.
 * Everything else -- ZAFX_LAYOUT_TF, |X| / |X|^2 and every other window in float64, compact rows, a d_out off the line grid, a
 * d_in off 16 bytes in float64, CQT kinds -- runs one zafx_execute per clip on the plan's stream ("per-clip <kernel>"). */
int zafx_execute_ragged(zafx_plan* plan, const void* d_in, const int64_t* in_offsets, const int64_t* lengths, void* d_out,
                        int64_t n_clips);
/* The center / sides extraction of n_clips stereo clips of different lengths in ONE launch (ZAFX_CENTER and ZAFX_CENTER_SIDES
 * plans only; last kernel "k_center_ragged"), enqueued on the plan's stream (asynchronous).  Offsets and lengths count sample
 * frames (one sample frame = L, R = 8 bytes): clip i is lengths[i] sample frames at sample frame in_offsets[i] of d_in -- clips
 * may lie back to back, each is padded with zeros of its own -- and its center goes to sample frame out_offsets[i] of d_out;
 * under ZAFX_CENTER_SIDES its sides follow directly behind, at out_offsets[i] + lengths[i] (the (2, N_i, 2) block of the
 * equal-length kind, one per clip).  Every clip's result is bit-identical to zafx_execute on that clip alone.  A clip of
 * length 0 is skipped: nothing of it is written.  The three host arrays are copied before return.  Rejected with a message:
 * n_clips < 0, negative lengths or offsets, a clip of 2^28 sample frames or more.  NOT checked: that the output blocks do not
 * overlap -- placing them is the caller's business.  d_in and d_out need 4-byte alignment only, as every float32 array (the opening
 * contract): a sample frame is read and written as one 8-byte piece, at the clip's own base plus a multiple of 8 bytes, whatever that base is
 * (k_center has no address test; tests/test_gpu_arena.py runs bases at 4 mod 8). */
int zafx_execute_center_ragged(zafx_plan* plan, const void* d_in, const int64_t* in_offsets, const int64_t* lengths, void* d_out,
                               const int64_t* out_offsets, int64_t n_clips);
/* The IMDCT of n_clips coefficient blocks of different frame counts, enqueued on the plan's stream (asynchronous; ZAFX_IMDCT plans only --
 * zafx_execute_ragged and zafx_plan_ragged_layout keep refusing the inverse kinds).  Block i is the (W/2, frames[i]) array of one clip at
 * element in_offsets[i] of d_coefs: W/2 rows at the pitch zafx_plan_row_pitch(plan, frames[i]) in ZAFX_LAYOUT_FT -- the layout a forward
 * ZAFX_MDCT plan's zafx_execute_ragged writes at the same row_align, so the output buffer of a ragged MDCT can be fed back as it lies --,
 * frames[i] x W/2 compact in ZAFX_LAYOUT_TF.  The pad columns of a block are never used; they may hold anything.  Clip i's
 * max((W/2) (frames[i] - 1) - 1, 0) samples (zaf.py:1182) go to element out_offsets[i] of d_out; a block of at most one frame writes nothing.
 * Every clip's result is bit-identical to zafx_execute on that block alone.  The three host arrays are copied before return.
 * Rejected with a message: another plan kind, n_clips < 0, a negative frame count or offset (with the clip's index).  NOT checked: that the
 * output ranges do not overlap -- placing them is the caller's business.
 * ONE launch (last kernel "k_imdct_ragged") for float32 plans in ZAFX_LAYOUT_FT at window 512, 1024 and 2048 when every block's pitch is a
 * multiple of 4 floats, every block is below 2^32 bytes and the batch gives fewer than 2^31 units; d_out and the output offsets need 4-byte alignment
 * only (a clip's bits do not depend on where it is put).  Everything else -- ZAFX_LAYOUT_TF, float64, window 4096 / 8192, windows up to
 * 256, Bluestein windows, compact pitches off the 4-float grid -- runs one zafx_execute per clip on the plan's stream and reports that
 * kernel's name.  ZAFX_RAGGED_IMDCT_NATIVE=0 in the environment keeps a batch off the one launch, as ZAFX_RAGGED_MDCT_NATIVE does for the
 * forward transform: a switch for measurements only (tools/ragged_rates.py --kinds imdct), read at every call, not part of the interface. */
int zafx_execute_imdct_ragged(zafx_plan* plan, const void* d_coefs, const int64_t* in_offsets, const int64_t* frames, void* d_out,
                              const int64_t* out_offsets, int64_t n_clips);
/* The inverse STFT of n_clips spectra of different frame counts, enqueued on the plan's stream (asynchronous; ZAFX_ISTFT plans only --
 * zafx_execute_ragged and zafx_plan_ragged_layout keep refusing the inverse kinds).  Block i is the (W, frames[i]) complex array -- (W/2 + 1,
 * frames[i]) for a one-sided plan -- of one clip at complex element in_offsets[i] of d_spec: rows at the pitch zafx_plan_row_pitch(plan,
 * frames[i]) in ZAFX_LAYOUT_FT -- the layout a ZAFX_STFT plan's zafx_execute_ragged writes at the same row_align and spectrum, so the output
 * buffer of a ragged STFT can be fed back as it lies --, frames[i] x rows compact in ZAFX_LAYOUT_TF.  The pad columns of a block are never
 * used; they may hold anything.  Clip i's max(frames[i] H - (W - H), 0) samples (zaf.py istft) go to float out_offsets[i] of d_out; a block
 * that gives no samples writes nothing.  Every clip's result is bit-identical to zafx_execute on that block alone; nothing outside the clips
 * is written.  The three host arrays are copied before return.  Rejected with a message: another plan kind, n_clips < 0, a negative frame
 * count or offset (with the clip's index), a window constant that is not set, a window whose COLA gain sum(window[0:W:H]) is zero.  NOT
 * checked: that the output ranges do not overlap -- placing them is the caller's business.
 * ONE launch (last kernel "k_istft_ragged") for float32 plans in ZAFX_LAYOUT_FT at a power-of-two window 256 ... 2048 (the k_istft_ft16
 * route) with ceil(W / H) - 1 < 16, when d_spec is 4-byte aligned, the batch gives fewer than 2^31 units and every block is below 2^31 bytes
 * counted as W rows -- W x pitch x 8 < 2^31: the kernel addresses a block through one buffer descriptor with signed 32-bit byte offsets, the
 * bound of the equal-length route; 16-byte gathers when d_spec is 8-byte aligned, 8-byte ones otherwise; d_out and the output offsets need
 * 4-byte alignment only (a clip's bits do not depend on where it is put).  Everything else -- ZAFX_LAYOUT_TF, float64, window 4096 / 8192,
 * windows below 256, Bluestein windows, hops with ceil(W / H) - 1 >= 16 -- runs one zafx_execute per clip on the plan's stream and reports that
 * kernel's name.  ZAFX_RAGGED_ISTFT_NATIVE=0 in the environment keeps a batch off the one launch and ZAFX_ISTFT_UNITS_PER_SLOT sets the units
 * per workgroup slot its cutting rule aims at: switches for measurements only (tools/ragged_rates.py --kinds istft), read at every call, not
 * part of the interface. */
int zafx_execute_istft_ragged(zafx_plan* plan, const void* d_spec, const int64_t* in_offsets, const int64_t* frames, void* d_out,
                              const int64_t* out_offsets, int64_t n_clips);
/* Bytes of ONE clip on the input and on the output side of the plan for `n_in` (as zafx_plan_out_dims; rows at the
 * plan's pitch): what a host array of n_clips clips must hold for zafx_run_host. */
int zafx_plan_clip_bytes(const zafx_plan* plan, int64_t n_in, int64_t* in_bytes, int64_t* out_bytes);
/* The host-array boundary of the reference (zaf.py:45: NumPy array in, NumPy array out) in one call: h_in -> HBM ->
 * transform -> h_out, in chunks of `chunk_clips` clips (0: chosen by the library, about 128 MB per chunk) through a
 * three-stage pipeline (upload stream, the plan's stream, download stream; two sets of plan-owned device staging buffers),
 * so that upload, kernel and download of neighbouring chunks overlap and the call runs at the rate of the slower PCIe
 * direction instead of the sum of the three.  Synchronous: returns when h_out
 * is complete.  Page-locked host arrays (zafx_host_alloc) transfer asynchronously at the PCIe rate; pageable ones work
 * and are staged by the runtime.  Serialise with other calls on the same plan. */
int zafx_run_host(zafx_plan* plan, const void* h_in, void* h_out, int64_t n_clips, int64_t n_in, int64_t chunk_clips);
/* HIP-event stopwatch on the plan's stream (the stream the kernels run on). */
int zafx_timer_start(zafx_plan* plan);
int zafx_timer_stop(zafx_plan* plan, float* elapsed_ms);
/* Name of the kernel family the plan was built for (fixed at zafx_plan_create / the last constant upload: the route a
 * geometry is expected to take). */
int zafx_plan_kernel_name(const zafx_plan* plan, char* buf, size_t buflen);
/* Name of the dominant kernel the LAST zafx_execute / zafx_run_host of this plan really launched (for matching rocprofv3
 * rows; the carry / band / generic forms are chosen per call from T, hop and the buffers' alignment); "" before the
 * first execute. */
int zafx_plan_last_kernel_name(const zafx_plan* plan, char* buf, size_t buflen);
/* The compute units the plan sizes its launches for (*in_use: the device's count, or fewer under ZAFX_COMPUTE_UNITS at zafx_plan_create) and
 * those of its device (*on_device). */
int zafx_plan_compute_units(const zafx_plan* plan, int* in_use, int* on_device);
/* The form of k_cqt the LAST zafx_execute of a float32 CQT / chroma plan launched (both carry the name k_cqt): 1 = the matrix-core contraction
 * (a numerically real kernel matrix whose columns lie in the lower half and whose segments fit the registers), 2 = the lane reduction
 * (every other matrix); 0 before the first launch and for every other plan.  Chosen anew after each upload of a CQT constant. */
int zafx_plan_cqt_form(const zafx_plan* plan, int* form);

/* Largest number of rows (n_bins) of a CQT kernel matrix that a float32 ZAFX_CQT / ZAFX_CHROMA plan of this fft_length
 * holds (k_cqt keeps the frame and the rows' bookkeeping in the 160 KB of LDS); 0 when fft_length itself is outside the
 * float32 kernels.  Larger kernels (and fft_length up to 131072) run as ZAFX_PRECISION_F64 plans. */
int zafx_cqt_max_bins(int fft_length, int* n_bins);

/* ---- PCM ingest: the step in front of the path ------------------------------ */
/* wavread's normalisation (zaf.py:1202: x / 2^(8*itemsize - 1)) and the channel mean every example
 * applies before the transforms (zaf.py:65: np.mean(audio_signal, 1)), on device:
 *   out[c][i] = mean_ch( in[c][i][ch] ) / 2^(8*sample_bytes - 1)
 * in: (n_clips, n_frames, n_channels) interleaved int16 (sample_bytes 2) or int32 (4); out: float32.
 * Enqueued on the plan's stream, so it is ordered before a following zafx_execute on that plan. */
int zafx_pcm_to_float(zafx_plan* plan, const void* d_pcm, void* d_out, int64_t n_clips, int64_t n_frames,
                      int n_channels, int sample_bytes);
/* The transform of integer PCM that is already on the device, in one call: d_pcm (n_clips, n_frames, n_channels) interleaved int16 / int32 ->
 * what zafx_execute writes for the normalised mono signal (zaf.py:1202 x / 2^(bits-1), zaf.py:65 mean over the channels, then the plan's
 * transform).  Plans whose kernel takes the integers in its own loads -- int16, one or two channels, into ZAFX_MEL / ZAFX_MFCC, ZAFX_STFT
 * (every spectrum kind) and ZAFX_MDCT at window_length 2048 in the reference layout -- read 2 bytes per sample and channel of HBM instead of 6 + 4; every other
 * plan converts into a float32 staging array it owns (zafx_pcm_to_float) and runs zafx_execute on that.  Kinds as zafx_run_host_pcm. */
int zafx_execute_pcm(zafx_plan* plan, const void* d_pcm, void* d_out, int64_t n_clips, int64_t n_frames, int n_channels, int sample_bytes);
/* zafx_execute_ragged for integer PCM that is already on the device (asynchronous, on the plan's stream): clip i is lengths[i] SAMPLE FRAMES
 * -- one int16 / int32 per channel: 2 bytes for int16 mono, the 4 bytes of one (left, right) pair for int16 stereo -- at sample frame
 * in_offsets[i] of the interleaved array d_pcm; its result -- what zafx_execute_ragged writes for the normalised mono clip (zaf.py:1202, :65)
 * -- goes to the block zafx_plan_ragged_layout(plan, lengths, ...) assigns, unchanged.  The two host arrays are copied before return.  Kinds:
 * those of zafx_execute_ragged (float32 plans; ZAFX_DCT, center / sides and the inverse kinds are refused with a message).  Checked in this
 * order: the plan, n_clips < 0, the kind, null arrays and pointers, negative lengths or offsets (with the clip's index), n_channels in [1, 64],
 * sample_bytes 2 or 4, the plan's precision.
 * ONE launch, the integers in the kernel's own loads (2 or 4 bytes per sample frame of HBM instead of 6 + 4; last kernel as the float
 * launches: "k_mel2_ragged", "k_stft_ft16_ragged", "k_mdct_ft32_ragged"): int16, one or two channels, a float32 plan in ZAFX_LAYOUT_FT at
 * window_length 2048 whose every clip has rows of whole 128-byte lines, d_out 128-byte aligned (as zafx_execute_ragged), and
 *   - ZAFX_MEL / ZAFX_MFCC (with_mel included) where zafx_execute_ragged runs them on k_mel2, ZAFX_STFT of every spectrum kind: an even hop,
 *     d_pcm 8-byte aligned, every in_offsets[i] even, every clip below 2^29 sample frames; lengths of either parity (every load of more than
 *     one sample lies inside its clip, the tail goes sample by sample);
 *   - ZAFX_MDCT: d_pcm 16-byte aligned, every offset and length a multiple of 4 sample frames, every clip below 2^28 sample frames.
 * Everything else -- int32, other channel counts, other windows, odd hops or offsets, ZAFX_CQT / ZAFX_CHROMA, d_out off the line grid --
 * converts first: the clip list is cut, in the order given, into groups of consecutive clips whose covered span of d_pcm (lowest offset
 * to highest end) fits the plan's float32 staging array under the scratch budget (1 GiB; ZAFX_SCRATCH_BUDGET_MB) -- a group has at
 * least one clip, and clips whose offsets are not increasing give smaller groups --, and every group is one zafx_pcm_to_float over its span and
 * one zafx_execute_ragged: the bits of zafx_execute_ragged on the normalised samples.  ZAFX_RAGGED_PCM_NATIVE=0 in the environment keeps
 * every batch on the convert-first route: a switch for measurements only (tools/ragged_rates.py --kinds mel_pcm,...), read at every call,
 * not part of the interface. */
int zafx_execute_ragged_pcm(zafx_plan* plan, const void* d_pcm, const int64_t* in_offsets, const int64_t* lengths, void* d_out,
                            int64_t n_clips, int n_channels, int sample_bytes);

/* zafx_run_host for integer PCM: h_pcm = (n_clips, n_frames, n_channels) interleaved int16 / int32 as wavread's source
 * holds them (zaf.py:1187-1204); every chunk crosses PCIe as integers (2 or 4 bytes per sample and channel instead of 4 per
 * float32 sample), is normalised and mixed down on the device in front of the transform, and the transform's result comes
 * back as from zafx_run_host.  Plans that take samples: STFT, MDCT, MEL, MFCC, CQT, CHROMA, DCT (float32). */
int zafx_run_host_pcm(zafx_plan* plan, const void* h_pcm, void* h_out, int64_t n_clips, int64_t n_frames, int n_channels,
                      int sample_bytes, int64_t chunk_clips);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI --------------------------------- */
/* The only collective on this path: broadcast of the shared constants (window,
 * filterbank, DCT matrix, CQT kernel) from `root`.  No reduction exists. */
int zafx_comm_unique_id(void* id128 /* 128 bytes out */);
int zafx_comm_create(zafx_comm** comm, int device, int rank, int n_ranks, const void* id128);
int zafx_comm_destroy(zafx_comm* comm);
/* Size of the communicator and this process's rank in it as RCCL reports them (ncclCommCount, ncclCommUserRank). */
int zafx_comm_count(zafx_comm* comm, int* n_ranks);
int zafx_comm_user_rank(zafx_comm* comm, int* rank);
int zafx_comm_broadcast_constants(zafx_comm* comm, zafx_plan* plan, int root);

#ifdef __cplusplus
}
#endif
#endif /* ZAFX_H */
