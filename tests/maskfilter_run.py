"""One launch of a fused mask-filter kernel for the cross-route tests (tests/test_gpu_accuracy.py, tests/test_gpu_windows.py,
tests/test_gpu_signals.py): any form of tests/maskfilter_cases.py, through its equal-length entry point or its ragged one, on device buffers,
into an output filled with NaN, the kernel asserted by name.  run(): the float32 entry points; run_pcm(): zafx_execute_masked_pcm and
zafx_execute_masked_pcm_ragged on int16 clips, to float32 or to int16."""
import numpy as np

import maskfilter_cases as mc

FILL = 0x7FC5A5A5   # a quiet NaN no kernel computes
FILL16 = 0x7A5B     # the same for an int16 output: a word the tests' clips do not filter to by chance in 64 places


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def laid(plan, family, m, n):
    """One clip's mask(s), (..., W/2 + 1, T), as the plan reads them, flat: "TF" (..., T, W/2 + 1) compact -- a stereo clip's two masks
    (T, 2, W/2 + 1), a frame's L row in front of its R row --; "FT" rows at the plan's pitch with NaN in the padding."""
    import zafx
    if family == "stereo" and np.ndim(m) == 3:
        return np.ascontiguousarray(np.transpose(m, (2, 0, 1)), np.float32).ravel()
    if plan.layout == zafx.LAYOUT_TF:
        return np.ascontiguousarray(np.swapaxes(m, -1, -2), np.complex64 if family == "complex" else np.float32).ravel()
    out = np.full((m.shape[0], plan.row_pitch(n)), np.nan, np.float32)
    out[:, :m.shape[1]] = m
    return out.ravel()


def run(form, w, clips, masks, rest, ragged, plan=None, refusal=None):
    """-> per clip its (rows, N_i) float32 result: the stems (one for the one-mask forms) and with `rest` the rest behind them; a stereo form's
    channels de-interleaved, y_L, y_R and with `rest` rest_L, rest_R.  Equal-length: every clip has the same length.  Every output word
    outside the clips' blocks must keep the fill.  plan: a plan of the caller's -- its window, its `rest`, the form's layout -- where the
    cached one of zafx.maskfilter_plan(w, rest, ...) will not do (a window replaced on a used plan: tests/test_gpu_constants.py).  refusal:
    words the library must refuse the call with, leaving every word of the filled output as it was -> None."""
    return _launch(form, w, clips, masks, rest, ragged, None, plan, refusal)


def run_pcm(form, w, clips, masks, rest, ragged, out, plan=None, refusal=None):
    """The same through the PCM entry points, form one of mc.PCM_FORMS: int16 clips, (N,) for "tf" and (N, 2) for the stereo forms, to
    `out` = np.float32 or np.int16 -> per clip its (rows, N_i) result of that dtype."""
    assert form in mc.PCM_FORMS and np.dtype(out) in (np.dtype(np.float32), np.dtype(np.int16)), (form, out)
    assert all(c.dtype == np.int16 for c in clips)
    return _launch(form, w, clips, masks, rest, ragged, np.dtype(out), plan, refusal)


def _enqueue(zafx, plan, refusal, call):
    """call() -> False; or, with `refusal`, True once the library has refused it in those words (anything else: an assertion)."""
    if refusal is None:
        call()
        return False
    try:
        call()
    except zafx.ZafxError as e:
        assert refusal in str(e), (refusal, str(e))
        return True
    raise AssertionError(f"the call ran where it must be refused: {refusal}")


def _launch(form, w, clips, masks, rest, ragged, pcm_out, plan, refusal=None):
    import zafx
    family, layout, row_align = mc.FORMS[form]
    if plan is None:
        plan = zafx.maskfilter_plan(w, rest=rest, layout=layout, row_align=row_align)
    else:
        assert plan.kind == (zafx.MASKFILTER_REST if rest else zafx.MASKFILTER) and (layout, row_align) == ("TF", 0) and plan.layout == zafx.LAYOUT_TF
    stereo = family == "stereo"
    mask_channels = mc.STEREO_DATA[form] if stereo else 1
    assert all(np.ndim(m) == (2 if mask_channels == 1 else 3) for m in masks) or family == "stems", (form, [np.shape(m) for m in masks])
    stems = len(masks[0]) if family == "stems" else 1
    blocks = stems + int(rest)      # a clip's output blocks, of N_i samples or, stereo, of N_i sample frames
    width = 2 if stereo else 1      # words per sample frame
    lengths = np.array([len(c) for c in clips], np.int64)
    flat = [laid(plan, family, m, len(c)) for c, m in zip(clips, masks)]
    in_offs = np.concatenate(([0], np.cumsum(lengths)))
    out_offs = blocks * in_offs
    if not ragged:
        assert len(set(lengths.tolist())) == 1
        mask_offs = np.concatenate(([0], np.cumsum([len(f) for f in flat])))
    elif family == "stems":
        mask_offs, layout_out = plan.stems_ragged_layout(lengths, stems)
        assert layout_out.tolist() == out_offs.tolist()
    elif stereo:
        mask_offs, layout_out = plan.stereo_ragged_layout(lengths, mask_channels)
        assert layout_out.tolist() == out_offs.tolist()
        assert mask_offs.tolist() == (mask_channels * plan.mask_ragged_layout(lengths)).tolist()
    else:
        mask_offs = plan.mask_ragged_layout(lengths)
    h_mask = np.full(max(int(mask_offs[-1]), 1), np.nan, flat[0].dtype if flat else np.float32)
    for f, lo, hi in zip(flat, mask_offs[:-1].tolist(), mask_offs[1:].tolist()):
        assert len(f) <= hi - lo, (form, len(f), hi - lo)
        h_mask[lo:lo + len(f)] = f
    in_dtype = np.float32 if pcm_out is None else np.int16
    x = np.concatenate([np.asarray(c, in_dtype).reshape(-1) for c in clips] + [np.zeros(2, in_dtype)])
    words = width * max(int(out_offs[-1]), 1) + 64
    if pcm_out is None or pcm_out == np.float32:
        h_out = np.full(words, FILL, np.uint32).view(np.float32)
    else:
        h_out = np.full(words, FILL16, np.int16)
    d_in, d_mask, d_out = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(h_mask), zafx.DeviceBuffer.from_host(h_out)
    try:
        def call():
            b, n = len(clips), int(lengths[0]) if len(lengths) else 0
            if pcm_out is not None and not ragged:
                plan.execute_masked_pcm(d_in, d_mask, d_out, b, n, width, mask_channels)
            elif pcm_out is not None:
                plan.execute_masked_pcm_ragged(d_in, in_offs[:-1], lengths, d_mask, mask_offs, d_out, out_offs[:-1], width, mask_channels)
            elif not ragged:
                if family == "real":
                    plan.execute_masked(d_in, d_mask, d_out, b, n)
                elif family == "stems":
                    plan.execute_masked_stems(d_in, d_mask, d_out, b, n, stems)
                elif stereo:
                    plan.execute_masked_stereo(d_in, d_mask, d_out, b, n, mask_channels)
                else:
                    plan.execute_masked_complex(d_in, d_mask, d_out, b, n)
            elif family == "real":
                plan.execute_masked_ragged(d_in, in_offs[:-1], lengths, d_mask, mask_offs, d_out, out_offs[:-1])
            elif family == "stems":
                plan.execute_masked_stems_ragged(d_in, in_offs[:-1], lengths, d_mask, mask_offs, d_out, out_offs[:-1], stems)
            elif stereo:
                plan.execute_masked_stereo_ragged(d_in, in_offs[:-1], lengths, d_mask, mask_offs, d_out, out_offs[:-1], mask_channels)
            else:
                plan.execute_masked_complex_ragged(d_in, in_offs[:-1], lengths, d_mask, mask_offs, d_out, out_offs[:-1])
        want = mc.PCM_KERNELS[width][int(ragged)] if pcm_out is not None else mc.KERNELS[family][int(ragged)]
        if _enqueue(zafx, plan, refusal, call):
            plan.sync()
            kept = d_out.download()
            assert (kept == FILL16).all() if kept.dtype == np.int16 else (bits(kept) == FILL).all(), (form, ragged, "a refused call wrote to the output")
            return None
        plan.sync()
        assert plan.last_kernel == want and plan.kernel_name == "k_maskfilter", (form, ragged, plan.last_kernel, want)
        got = d_out.download()
    finally:
        for buf in (d_in, d_mask, d_out):
            buf.free()
    behind = got[width * int(out_offs[-1]):]
    assert (behind == FILL16).all() if got.dtype == np.int16 else (bits(behind) == FILL).all(), (form, ragged, "written behind the output")
    res = []
    for lo, hi, n in zip(out_offs[:-1].tolist(), out_offs[1:].tolist(), lengths.tolist()):
        block = got[width * lo:width * hi]
        # (stereo: (blocks, N, 2) interleaved -> (2 blocks, N): y_L, y_R, rest_L, rest_R)
        res.append(np.ascontiguousarray(block.reshape(blocks, n, 2).transpose(0, 2, 1)).reshape(2 * blocks, n) if stereo else block.reshape(blocks, n))
    return res
