"""One launch of a fused mask-filter kernel for the cross-route tests (tests/test_gpu_accuracy.py, tests/test_gpu_windows.py,
tests/test_gpu_signals.py): any form of tests/maskfilter_cases.py, through its equal-length entry point or its ragged one, on device buffers,
into an output filled with NaN, the kernel asserted by name."""
import numpy as np

import maskfilter_cases as mc

FILL = 0x7FC5A5A5   # a quiet NaN no kernel computes


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def laid(plan, family, m, n):
    """One clip's mask(s), (..., W/2 + 1, T), as the plan reads them, flat: "TF" (..., T, W/2 + 1) compact; "FT" rows at the plan's pitch with
    NaN in the padding."""
    import zafx
    if plan.layout == zafx.LAYOUT_TF:
        return np.ascontiguousarray(np.swapaxes(m, -1, -2), np.complex64 if family == "complex" else np.float32).ravel()
    out = np.full((m.shape[0], plan.row_pitch(n)), np.nan, np.float32)
    out[:, :m.shape[1]] = m
    return out.ravel()


def run(form, w, clips, masks, rest, ragged):
    """-> per clip its (rows, N_i) float32 result: the stems (one for the one-mask forms) and with `rest` the rest behind them.  Equal-length:
    every clip has the same length.  Every output word outside the clips' blocks must keep the fill."""
    import zafx
    family, layout, row_align = mc.FORMS[form]
    plan = zafx.maskfilter_plan(w, rest=rest, layout=layout, row_align=row_align)
    stems = len(masks[0]) if family == "stems" else 1
    rows = stems + int(rest)
    lengths = np.array([len(c) for c in clips], np.int64)
    flat = [laid(plan, family, m, len(c)) for c, m in zip(clips, masks)]
    in_offs = np.concatenate(([0], np.cumsum(lengths)))
    out_offs = rows * in_offs
    if not ragged:
        assert len(set(lengths.tolist())) == 1
        mask_offs = np.concatenate(([0], np.cumsum([len(f) for f in flat])))
    elif family == "stems":
        mask_offs, layout_out = plan.stems_ragged_layout(lengths, stems)
        assert layout_out.tolist() == out_offs.tolist()
    else:
        mask_offs = plan.mask_ragged_layout(lengths)
    h_mask = np.full(max(int(mask_offs[-1]), 1), np.nan, flat[0].dtype if flat else np.float32)
    for f, lo, hi in zip(flat, mask_offs[:-1].tolist(), mask_offs[1:].tolist()):
        assert len(f) <= hi - lo, (form, len(f), hi - lo)
        h_mask[lo:lo + len(f)] = f
    x = np.concatenate(list(clips) + [np.zeros(1, np.float32)]).astype(np.float32)
    words = max(int(out_offs[-1]), 1) + 64
    d_in, d_mask = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(h_mask)
    d_out = zafx.DeviceBuffer.from_host(np.full(words, FILL, np.uint32).view(np.float32))
    try:
        if not ragged:
            b, n = len(clips), int(lengths[0])
            if family == "real":
                plan.execute_masked(d_in, d_mask, d_out, b, n)
            elif family == "stems":
                plan.execute_masked_stems(d_in, d_mask, d_out, b, n, stems)
            else:
                plan.execute_masked_complex(d_in, d_mask, d_out, b, n)
        elif family == "real":
            plan.execute_masked_ragged(d_in, in_offs[:-1], lengths, d_mask, mask_offs, d_out, out_offs[:-1])
        elif family == "stems":
            plan.execute_masked_stems_ragged(d_in, in_offs[:-1], lengths, d_mask, mask_offs, d_out, out_offs[:-1], stems)
        else:
            plan.execute_masked_complex_ragged(d_in, in_offs[:-1], lengths, d_mask, mask_offs, d_out, out_offs[:-1])
        plan.sync()
        want = mc.KERNELS[family][int(ragged)]
        assert plan.last_kernel == want and plan.kernel_name == "k_maskfilter", (form, ragged, plan.last_kernel, want)
        got = d_out.download()
    finally:
        for buf in (d_in, d_mask, d_out):
            buf.free()
    assert (bits(got[int(out_offs[-1]):]) == FILL).all(), (form, ragged, "written behind the output")
    return [got[lo:hi].reshape(rows, n) for lo, hi, n in zip(out_offs[:-1].tolist(), out_offs[1:].tolist(), lengths.tolist())]
