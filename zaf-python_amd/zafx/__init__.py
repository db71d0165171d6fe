"""zafx -- MI355X-native drop-in for the windowed-transform path of zaf.py.

    import zafx as zaf          # same signatures as zafarrafii/Zaf-Python for this path
    X = zaf.stft(x, w, 1024)    # runs on the GPU through libzafx.so (hand-written HIP)

Drop-in functions (zaf.py signatures, float64 / complex128 results):
    stft, istft, melfilterbank, melspectrogram, mfcc, cqtkernel, cqtspectrogram,
    cqtchromagram, mdct, imdct, dct, dst
The center / sides example of zaf.istft's docstring (stereo STFT, masks, ISTFT, subtraction) in one kernel:
    centersides ((N, 2) -> (center, sides)), centersides_batch ((B, N, 2) float32), center_plan;
    centersides_ragged (a sequence of (N_i, 2) clips of different lengths in one launch), pack_ragged_stereo, Plan.execute_center_ragged
The same with a mask of the caller's (STFT, real mask, ISTFT of mono clips in one kernel; zaf.py:185-195):
    maskfilter ((N,), (W/2+1, T) -> (N,)), maskfilter_batch ((B, N), (B, W/2+1, T) float32), maskfilter_plan, Plan.execute_masked / Plan.mask_shape
    maskfilter_ragged (sequences of (N_i,) clips and (W/2+1, T_i) masks of different lengths in one launch), pack_ragged_masks,
    Plan.mask_ragged_layout / Plan.execute_masked_ragged
    maskfilter_stems ((N,), (S, W/2+1, T) -> (S, N)), maskfilter_stems_batch ((B, N), (B, S, W/2+1, T) float32 -> (B, S, N)): S = 1 .. 8 masks per
    clip over one forward transform in one launch; Plan.execute_masked_stems / Plan.stems_mask_shape / Plan.stems_out_shape
    maskfilter_stems_ragged (sequences of (N_i,) clips and (S, W/2+1, T_i) masks of different lengths -> a list of (S, N_i) in one launch),
    pack_ragged_stems_masks, Plan.stems_ragged_layout / Plan.execute_masked_stems_ragged
    maskfilter_complex ((N,), complex (W/2+1, T) -> (N,)), maskfilter_complex_batch ((B, N), (B, W/2+1, T) complex64): a complex mask, extended
    to its Hermitian mirror, in one kernel; maskfilter_complex_ragged (clips and masks of different lengths in one launch),
    pack_ragged_complex_masks, Plan.execute_masked_complex / Plan.execute_masked_complex_ragged
    maskfilter_stereo ((N, 2), (W/2+1, T) or (2, W/2+1, T) -> (N, 2)), maskfilter_stereo_batch ((B, N, 2), (B, W/2+1, T) or (B, 2, W/2+1, T)):
    interleaved stereo clips under one mask for both channels or one per channel, in one kernel; maskfilter_stereo_ragged (clips and masks
    of different lengths in one launch), pack_ragged_stereo_masks, Plan.execute_masked_stereo / Plan.execute_masked_stereo_ragged /
    Plan.stereo_mask_shape / Plan.stereo_out_shape / Plan.stereo_ragged_layout
    maskfilter_pcm (int16 (N,) or (N, 2) -> int16 or float32), maskfilter_pcm_batch ((B, N) or (B, N, 2) int16), maskfilter_pcm_ragged: the
    mono and the stereo mask filter on 16-bit PCM, the integers read and written by the kernel (s / 32768 in; rint, saturating, out; the rest
    in integers); Plan.execute_masked_pcm / Plan.execute_masked_pcm_ragged
Batched extension ((clips, samples) in, float32 / complex64 out):
    stft_batch, istft_batch, mdct_batch, imdct_batch, melspectrogram_batch, mfcc_batch,
    cqtspectrogram_batch, cqtchromagram_batch, dct_batch, dst_batch, mel_mfcc_batch (melspectrogram + mfcc from one set of transforms);
    the same from interleaved int16 / int32 PCM:
    stft_pcm_batch, mdct_pcm_batch, melspectrogram_pcm_batch, mfcc_pcm_batch, cqtspectrogram_pcm_batch, cqtchromagram_pcm_batch
Ragged batches (a sequence of 1-D clips of different lengths in, a list of per-clip arrays out -- views of one result buffer -- in one
launch where the library has the kernel):
    stft_ragged, mdct_ragged, melspectrogram_ragged, mfcc_ragged, mel_mfcc_ragged; pack_ragged (the packed array they upload);
    Plan.ragged_layout / Plan.execute_ragged on device buffers (every forward kind that takes samples);
    imdct_ragged (a sequence of (W/2, T_i) coefficient blocks -- mdct_ragged's views as they lie -- back to clips), Plan.execute_imdct_ragged;
    istft_ragged (a sequence of (W, T_i) spectra -- stft_ragged's views as they lie -- back to clips), Plan.execute_istft_ragged;
    the forward ones from int16 / int32 PCM clips, (N_i,) or (N_i, C): stft_pcm_ragged, mdct_pcm_ragged, melspectrogram_pcm_ragged,
    mfcc_pcm_ragged, mel_mfcc_pcm_ragged; pack_ragged_pcm; Plan.execute_ragged_pcm on device buffers
Device-resident API: Plan, DeviceBuffer, Comm, *_plan factories, shard helpers; one process per GPU: launch.Rendezvous,
spawn_ranks (file rendezvous + self-launcher, no torch.distributed).
"""
from ._lib import (CENTER, CENTER_SIDES, CHROMA, CQT, DCT, IMDCT, ISTFT, LAYOUT_FT, LAYOUT_TF, LINEAR, MASKFILTER, MASKFILTER_MAX_STEMS, MASKFILTER_REST, MDCT, MEL, MFCC, STFT, ZafxError,
                   center_tile_frames, device_count, device_name, library_path, maskfilter_tile_transforms)
from .constants import cqtkernel, dct2_rows, dct_matrix, dst_matrix, hamming, kaiser_bessel_derived, melfilterbank, sine
from .core import (Comm, DeviceBuffer, Plan, center_plan, centersides, centersides_batch, maskfilter, maskfilter_batch, maskfilter_plan, maskfilter_stems, maskfilter_stems_batch, maskfilter_complex, maskfilter_complex_batch, maskfilter_stereo, maskfilter_stereo_batch, maskfilter_pcm, maskfilter_pcm_batch, clear_plan_cache, cqt_plan, cqtchromagram, cqtchromagram_batch, dct, dct_batch, dst,
                   dst_batch, linear_plan, dct_plan, dct_fft_length,
                   cqtspectrogram, cqtspectrogram_batch, imdct, imdct_batch, istft, istft_batch, istft_plan, mdct,
                   mdct_batch, mdct_plan, mel_plan, melspectrogram, melspectrogram_batch, mfcc, mfcc_batch, pcm_to_mono, pinned_empty,
                   get_precision, set_precision, stft, stft_batch, stft_pcm_batch, stft_plan, mdct_pcm_batch, melspectrogram_pcm_batch, mfcc_pcm_batch,
                   cqtspectrogram_pcm_batch, cqtchromagram_pcm_batch, mel_mfcc_batch, mel_mfcc_pcm_batch, mel_mfcc_supported, set_row_padding, get_row_padding,
                   stft_ragged, mdct_ragged, melspectrogram_ragged, mfcc_ragged, mel_mfcc_ragged, pack_ragged, centersides_ragged, pack_ragged_stereo, maskfilter_ragged, pack_ragged_masks, maskfilter_stems_ragged, pack_ragged_stems_masks, maskfilter_complex_ragged, pack_ragged_complex_masks, maskfilter_stereo_ragged, pack_ragged_stereo_masks, maskfilter_pcm_ragged, imdct_ragged, istft_ragged,
                   stft_pcm_ragged, mdct_pcm_ragged, melspectrogram_pcm_ragged, mfcc_pcm_ragged, mel_mfcc_pcm_ragged, pack_ragged_pcm)
from .launch import Rendezvous, rank_env, spawn_ranks
from .shard import clip_range, run_sharded, shard_sizes

__version__ = "0.1.0"
