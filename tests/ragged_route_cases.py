"""The calls of tests/test_gpu_ragged_routes.py, tests/test_routes_host.py and tests/golden/make_ragged_route_golden.py: one per side of every
branch the ragged entry points take -- zafx_execute_ragged, zafx_execute_ragged_pcm, zafx_execute_imdct_ragged, zafx_execute_istft_ragged
(zaf-python_amd/csrc/zafx_routes.hpp, ragged_route and the two *_ragged_block predicates).

A case is plain data (`case(...)`, a superset of route_cases.case).  Every batch is three clips.  A forward clip has at least one frame
(zafx_plan_out_dims), so the forward batches are clips of 0 samples (1 frame; the CQT: 0 frames), one hop (2 frames; the CQT: 1) and 32 hops
(33 frames); the inverse batches are blocks of 0, 1 and 33 frames.  The clips lie 8 elements apart in the input array, so every default
offset and length is a multiple of 4; `shift` moves the second clip, `short` shortens the third.  Two things are made of a case:

  * call_line(c)   the batch as the host program tests/host_emu/routes_emu reads it (its ragged form) -- arithmetic only, no GPU;
  * record(name)   the plan from the package's own factory, one call with both arrays carved out of arenas (tests/arena.py) at the case's
                   byte offsets -> [last_kernel, SHA-256 of the whole output arena, the `aligned` flag the parent's conditions give a native
                   forward launch (None elsewhere), whether the int16 launch takes an integer batch (None: no integer batch)], or
                   ["refused", the message, None, None].

Inputs are seeded; this file imports the package only, never the oracle."""
import hashlib
import os
import zlib

import numpy as np

import arena
import route_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GAP = 8
INVERSE_FRAMES = (0, 1, 33)
ENTRIES = {"ragged": 0, "pcm": 0, "imdct": 1, "istft": 2}
SWITCHES = ("ZAFX_RAGGED_MDCT_NATIVE", "ZAFX_RAGGED_F64_NATIVE", "ZAFX_RAGGED_PCM_NATIVE", "ZAFX_RAGGED_IMDCT_NATIVE", "ZAFX_RAGGED_ISTFT_NATIVE")
NATIVE_FORWARD = ("k_stft_ft16_ragged", "k_mel2_ragged", "k_mdct_ft32_ragged")


def out_itemsize(c):
    real = 8 if c["f64"] else 4
    return 2 * real if c["family"] == "stft" and c["spectrum"] in (False, True) else real


def case(family, w, hop=None, spectrum=False, layout="FT", lines=True, f64=False, filters=0, ncoef=0, also_mel=False, in_delta=0, out_delta=0,
         shift=0, short=0, off=None, entry=None, channels=0, sample_bytes=0, cqt=False):
    """lines: rows padded to whole 128-byte lines (the inverses: to the 4-float / 2-complex grid their gathers want); off: the switch set to 0."""
    c = rc.case(family, w, hop, spectrum, layout=layout, in_delta=in_delta, out_delta=out_delta, filters=filters, ncoef=ncoef, pcm=channels > 0)
    c.update(f64=f64, also_mel=also_mel, shift=shift, short=short, off=off, channels=channels, sample_bytes=sample_bytes,
             entry=entry or (family if family in ("imdct", "istft") else "pcm" if channels else "ragged"))
    if layout == "FT" and lines:
        c["row_align"] = 4 if family in ("imdct", "istft") else 128 // out_itemsize(c)
    return c


def _cases():
    c = {}
    # ---- zafx_execute_ragged, float32 STFT
    for w in (256, 512, 1024, 2048):
        for spec, tag in ((False, "two"), (True, "one"), ("magnitude", "mag"), ("power", "pow")):
            c[f"stft_{w}_{tag}"] = case("stft", w, w // 2, spec)
    c["stft_2048_two_compact"] = case("stft", 2048, 1024, lines=False)
    c["stft_2048_mag_compact"] = case("stft", 2048, 1024, "magnitude", lines=False)
    c["stft_2048_tf"] = case("stft", 2048, 1024, layout="TF")
    c["stft_4096_two"] = case("stft", 4096, 2048)
    c["stft_bluestein_1000"] = case("stft", 1000, 500)
    c["stft_2048_two_out64"] = case("stft", 2048, 1024, out_delta=64)
    for spec, tag in ((False, "two"), ("magnitude", "mag")):   # the flag flips, the name stays
        c[f"stft_2048_{tag}_oddlen"] = case("stft", 2048, 1024, spec, short=1)
        c[f"stft_2048_{tag}_oddoff"] = case("stft", 2048, 1024, spec, shift=1)
        c[f"stft_2048_{tag}_x4"] = case("stft", 2048, 1024, spec, in_delta=4)
    c["stft_2048_two_oddhop"] = case("stft", 2048, 1023)
    # ---- zafx_execute_ragged, float32 mel / MFCC
    c["mel_2048"] = case("mel", 2048, 1024, filters=40)
    c["mfcc_2048"] = case("mfcc", 2048, 1024, filters=40, ncoef=13)
    c["mfcc_2048_with_mel"] = case("mfcc", 2048, 1024, filters=40, ncoef=13, also_mel=True)
    c["mfcc_2048_unpacked"] = case("mfcc", 2048, 1024, filters=200, ncoef=13)   # (more than 8 blocks of filters: no DCT table for k_mel2)
    c["mel_2048_300"] = case("mel", 2048, 1024, filters=300)
    c["mel_2048_compact"] = case("mel", 2048, 1024, filters=40, lines=False)
    c["mel_2048_oddoff"] = case("mel", 2048, 1024, filters=40, shift=1)
    c["mel_1024"] = case("mel", 1024, 512, filters=40)
    # ---- zafx_execute_ragged, float32 MDCT
    for w in (512, 1024, 2048):
        c[f"mdct_{w}"] = case("mdct", w)
    c["mdct_2048_off2"] = case("mdct", 2048, shift=2)
    c["mdct_2048_len2"] = case("mdct", 2048, short=2)
    c["mdct_2048_x8"] = case("mdct", 2048, in_delta=8)
    c["mdct_2048_env0"] = case("mdct", 2048, off="ZAFX_RAGGED_MDCT_NATIVE")
    c["mdct_4096"] = case("mdct", 4096)
    c["mdct_2048_compact"] = case("mdct", 2048, lines=False)
    c["mdct_2048_tf"] = case("mdct", 2048, layout="TF")
    # ---- zafx_execute_ragged, float64
    c["f64_stft_two"] = case("stft", 2048, 1024, f64=True)
    c["f64_stft_one"] = case("stft", 2048, 1024, True, f64=True)
    c["f64_mdct"] = case("mdct", 2048, f64=True)
    c["f64_mel"] = case("mel", 2048, 1024, filters=40, f64=True)
    c["f64_mfcc"] = case("mfcc", 2048, 1024, filters=40, ncoef=13, f64=True)
    c["f64_stft_mag"] = case("stft", 2048, 1024, "magnitude", f64=True)
    c["f64_stft_1024"] = case("stft", 1024, 512, f64=True)
    c["f64_stft_x8"] = case("stft", 2048, 1024, f64=True, in_delta=8)
    c["f64_stft_env0"] = case("stft", 2048, 1024, f64=True, off="ZAFX_RAGGED_F64_NATIVE")
    c["f64_mdct_env0"] = case("mdct", 2048, f64=True, off="ZAFX_RAGGED_F64_NATIVE")
    # ---- zafx_execute_ragged, CQT / chromagram
    c["cqt"] = case("cqt", 0, 80, cqt=True)
    c["chroma"] = case("chroma", 0, 80, cqt=True)
    # ---- zafx_execute_ragged_pcm
    for ch in (1, 2):
        c[f"pcm_stft_one_c{ch}"] = case("stft", 2048, 1024, True, channels=ch, sample_bytes=2)
        c[f"pcm_mag_c{ch}"] = case("stft", 2048, 1024, "magnitude", channels=ch, sample_bytes=2)
        c[f"pcm_mel_c{ch}"] = case("mel", 2048, 1024, filters=40, channels=ch, sample_bytes=2)
        c[f"pcm_mdct_c{ch}"] = case("mdct", 2048, channels=ch, sample_bytes=2)
    c["pcm_stft_oddlen"] = case("stft", 2048, 1024, True, channels=1, sample_bytes=2, short=1)   # (int16 wants even offsets only)
    c["pcm_stft_oddoff"] = case("stft", 2048, 1024, True, channels=1, sample_bytes=2, shift=1)
    c["pcm_mel_oddoff"] = case("mel", 2048, 1024, filters=40, channels=1, sample_bytes=2, shift=1)
    c["pcm_stft_p4"] = case("stft", 2048, 1024, True, channels=1, sample_bytes=2, in_delta=4)
    c["pcm_stft_1024"] = case("stft", 1024, 512, True, channels=1, sample_bytes=2)
    c["pcm_stft_int32"] = case("stft", 2048, 1024, True, channels=1, sample_bytes=4)
    c["pcm_stft_c3"] = case("stft", 2048, 1024, True, channels=3, sample_bytes=2)
    c["pcm_stft_env0"] = case("stft", 2048, 1024, True, channels=1, sample_bytes=2, off="ZAFX_RAGGED_PCM_NATIVE")
    c["pcm_mdct_off2"] = case("mdct", 2048, channels=1, sample_bytes=2, shift=2)
    c["pcm_mdct_p8"] = case("mdct", 2048, channels=1, sample_bytes=2, in_delta=8)
    c["pcm_mdct_1024"] = case("mdct", 1024, channels=1, sample_bytes=2)
    c["pcm_mdct_mdct_env0"] = case("mdct", 2048, channels=1, sample_bytes=2, off="ZAFX_RAGGED_MDCT_NATIVE")   # (the int16 MDCT ignores it)
    c["pcm_mdct_env0"] = case("mdct", 2048, channels=1, sample_bytes=2, off="ZAFX_RAGGED_PCM_NATIVE")
    # ---- zafx_execute_imdct_ragged
    c["imdct_512"] = case("imdct", 512)
    c["imdct_2048"] = case("imdct", 2048)
    c["imdct_2048_pitch33"] = case("imdct", 2048, lines=False)
    c["imdct_2048_tf"] = case("imdct", 2048, layout="TF")
    c["imdct_4096"] = case("imdct", 4096)
    c["imdct_2048_f64"] = case("imdct", 2048, f64=True)
    c["imdct_2048_env0"] = case("imdct", 2048, off="ZAFX_RAGGED_IMDCT_NATIVE")
    # ---- zafx_execute_istft_ragged
    c["istft_256"] = case("istft", 256, 128)
    c["istft_2048_two"] = case("istft", 2048, 1024)
    c["istft_2048_one"] = case("istft", 2048, 1024, True)
    c["istft_2048_s4"] = case("istft", 2048, 1024, in_delta=4)   # (d_spec off 8 bytes: the 8-byte gather, the name stays)
    c["istft_2048_halo31"] = case("istft", 2048, 64)
    c["istft_2048_tf"] = case("istft", 2048, 1024, layout="TF")
    c["istft_4096"] = case("istft", 4096, 2048)
    c["istft_2048_f64"] = case("istft", 2048, 1024, f64=True)
    c["istft_2048_env0"] = case("istft", 2048, 1024, off="ZAFX_RAGGED_ISTFT_NATIVE")
    return c


CASES = _cases()


# ------------------------------------------------------------------------------------------------------------ arithmetic (no GPU)
def is_inverse(c):
    return c["entry"] in ("imdct", "istft")


def is_cqt(c):
    return c["family"] in ("cqt", "chroma")


def lengths(c):
    """Forward: samples (int16: sample frames) of the three clips; inverse: frames of the three blocks."""
    if is_inverse(c):
        return list(INVERSE_FRAMES)
    h = c["hop"]
    return [0, h, (33 if is_cqt(c) else 32) * h - c["short"]]


def frames(c):
    if is_inverse(c):
        return list(INVERSE_FRAMES)
    h = c["hop"]
    return [n // h if is_cqt(c) else -(-n // h) + 1 for n in lengths(c)]


def rows(c):
    """Rows of an inverse case's input block."""
    return c["W"] // 2 if c["family"] == "imdct" else c["W"] // 2 + 1 if c["spectrum"] else c["W"]


def in_offsets(c):
    n = lengths(c)
    if is_inverse(c):
        sizes = [rows(c) * (rc.pitch(c, t) if c["layout"] == "FT" else t) for t in n]
        return [0, sizes[0] + GAP, sizes[0] + sizes[1] + 2 * GAP]
    return [0, GAP + c["shift"], n[1] + 2 * GAP]


def in_elems(c):
    n = lengths(c)
    last = rows(c) * (rc.pitch(c, n[2]) if c["layout"] == "FT" else n[2]) if is_inverse(c) else n[2]
    return in_offsets(c)[2] + last + GAP


def out_lens(c):
    return [rc.out_len(dict(c, frames=t)) for t in INVERSE_FRAMES]


def out_offsets(c):
    """Inverse: where the blocks' samples go -- 8 apart; -> (offsets, elements in all)."""
    n = out_lens(c)
    return [0, n[0] + GAP, n[0] + n[1] + 2 * GAP], n[0] + n[1] + n[2] + 2 * GAP


def _aligned(c, base, offs, pcm):
    n = lengths(c)
    if c["family"] == "mdct":
        return base % 16 == 0 and all(o % 4 == 0 for o in offs) and all(k % 4 == 0 for k in n)
    return c["hop"] % 2 == 0 and base % 8 == 0 and all(o % 2 == 0 for o in offs) and (pcm or all(k % 2 == 0 for k in n))


def pcm_taken(c):
    """Does the one int16 launch of zafx_execute_ragged_pcm take the batch (the parent's conditions, zafx_capi.cpp before the move)?  None:
    no integer batch.  The batches it leaves are converted into the plan's staging array and run as a float batch there."""
    if not c["channels"]:
        return None
    base, offs = 256 + c["in_delta"], in_offsets(c)
    if c["sample_bytes"] != 2 or c["channels"] > 2 or c["off"] == "ZAFX_RAGGED_PCM_NATIVE":
        return 0
    if c["layout"] != "FT" or c["row_align"] * out_itemsize(c) % 128 or c["out_delta"] % 128 or c["W"] != 2048:
        return 0
    return int(_aligned(c, base, offs, True) and (c["family"] != "mdct" or base % 4 == 0))


def expected_aligned(c):
    """The `aligned` argument the parent's execute_ragged_checked hands a native forward launch (zafx_capi.cpp before the move).  An integer
    batch the int16 launch does not take runs as a float batch on the staging array: on 256 bytes, offsets counted from the lowest."""
    offs = in_offsets(c)
    if c["channels"] and not pcm_taken(c):
        return int(_aligned(c, 256, [o - min(offs) for o in offs], False))
    return int(_aligned(c, 256 + c["in_delta"], offs, c["channels"] > 0))


def mel2_packed(c):
    return c["family"] != "mfcc" or (c["ncoef"] <= 32 and -(-c["filters"] // 16) <= 8)


def f64_tiled(c):
    """zafx_f64.hip's three *_f64_tiled predicates for the plans of this file: W = 2048 in the reference layout, the complex kinds."""
    return int(c["f64"] and c["W"] == 2048 and c["layout"] == "FT" and (c["family"] != "stft" or c["spectrum"] in (False, True)))


def call_line(c, as_float=False, in_addr=None, offsets=None, lens=None, frms=None, **fields):
    """The batch as one line of routes_emu's ragged form.  as_float: an integer batch as the float batch it becomes on the plan's staging
    array (on 256 bytes, offsets counted from the lowest).  The other overrides: d_in's address, the per-clip lists (any number of clips) and
    any field of the line (tables=0: a plan without its twiddle tables)."""
    bluestein = c["W"] & (c["W"] - 1) != 0
    plan = dict(c, W=1 << c["W"].bit_length() if bluestein else c["W"] or 4096)
    offsets = in_offsets(c) if offsets is None else offsets
    if as_float:
        in_addr, offsets = 256, [o - min(offsets) for o in offsets]
    lens = lengths(c) if lens is None else lens
    frms = frames(c) if frms is None else frms
    head = rc.call_line(plan, n_clips=len(lens), n=0, frames=0, in_addr=256 + c["in_delta"] if in_addr is None else in_addr)
    off = c["off"]
    f = dict(entry=ENTRIES[c["entry"]], f64=int(c["f64"]), bluestein=int(bluestein), mel2=int(mel2_packed(c)), f64_tiled=f64_tiled(c),
             channels=0 if as_float else c["channels"], sample_bytes=0 if as_float else c["sample_bytes"],
             env_pcm=int(off != "ZAFX_RAGGED_PCM_NATIVE"), env_mdct=int(off != "ZAFX_RAGGED_MDCT_NATIVE"), env_f64=int(off != "ZAFX_RAGGED_F64_NATIVE"),
             env_inverse=int(off not in ("ZAFX_RAGGED_IMDCT_NATIVE", "ZAFX_RAGGED_ISTFT_NATIVE")))
    f.update(fields)
    lists = dict(offsets=offsets, lengths=lens, frames=frms)
    return head + " " + " ".join(f"{k}={v}" for k, v in f.items()) + " " + " ".join(f"{k}={','.join(str(int(v)) for v in vs)}" for k, vs in lists.items())


# ------------------------------------------------------------------------------------------------------------ the running half (GPU)
def make_plan(c):
    import scipy.sparse
    import zafx
    w, h = c["W"], c["hop"]
    if is_cqt(c):
        ck = scipy.sparse.csr_matrix(np.load(os.path.join(GOLDEN, "tiny.npz"))["ck_dense"])
        return zafx.cqt_plan(4000, 50, ck, 12 if c["family"] == "chroma" else None)
    if c["family"] == "stft":
        return zafx.stft_plan(zafx.hamming(w), h, layout=c["layout"], onesided=c["spectrum"], row_align=c["row_align"], f64=c["f64"])
    if c["family"] == "istft":
        return zafx.istft_plan(zafx.hamming(w), h, layout=c["layout"], onesided=c["spectrum"], row_align=c["row_align"], f64=c["f64"])
    if c["family"] in ("mdct", "imdct"):
        return zafx.mdct_plan(zafx.sine(w), layout=c["layout"], inverse=c["family"] == "imdct", row_align=c["row_align"], f64=c["f64"])
    return zafx.mel_plan(zafx.hamming(w), h, zafx.melfilterbank(rc.FS, w, c["filters"]), c["ncoef"] or None, layout=c["layout"], row_align=c["row_align"],
                         f64=c["f64"], also_mel=c["also_mel"])


def run(c, plan, tag):
    """One call at the case's addresses -> the whole output arena's bytes (guards, row padding and the gaps between blocks included)."""
    import zafx
    offs, n = np.array(in_offsets(c), np.int64), np.array(lengths(c), np.int64)
    if c["channels"]:
        dtype = np.int16 if c["sample_bytes"] == 2 else np.int32
        x = rc.noise(tag, (in_elems(c), c["channels"]) if c["channels"] > 1 else (in_elems(c),), np.int16).astype(dtype)
    else:
        x = rc.noise(tag, (in_elems(c),), plan.in_dtype)
    if is_inverse(c):
        out_offs, out_elems = out_offsets(c)
        out_offs = np.array(out_offs, np.int64)
        call = plan.execute_imdct_ragged if c["entry"] == "imdct" else plan.execute_istft_ragged
        launch = lambda d_in, d_out: (call(d_in, offs, n, d_out, out_offs), plan.sync())
    else:
        out_elems = int(plan.ragged_layout(n)[0][-1])
        if c["channels"]:
            launch = lambda d_in, d_out: (plan.execute_ragged_pcm(d_in, offs, n, d_out, c["channels"]), plan.sync())
        else:
            launch = lambda d_in, d_out: (plan.execute_ragged(d_in, offs, n, d_out), plan.sync())
    guard = arena.guard_bytes(x.nbytes, out_elems * plan.out_dtype.itemsize)
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        if c["off"]:
            os.environ[c["off"]] = "0"
        got, _ = arena.run_in_arena(zafx, x, plan.out_dtype, out_elems, guard, c["in_delta"], c["out_delta"], launch)
    finally:
        os.environ.pop(c["off"] or "", None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return np.asarray(got, np.uint8).tobytes()


def record(name):
    """-> [last_kernel, SHA-256 of the output arena, expected_aligned of a native forward launch or None, pcm_taken], or
    ["refused", message, None, None]."""
    c = CASES[name]
    try:
        plan = make_plan(c)
        out = run(c, plan, zlib.crc32(name.encode()))
    except (RuntimeError, ValueError) as e:
        return ["refused", str(e), None, None]
    kernel = plan.last_kernel
    return [kernel, hashlib.sha256(out).hexdigest(), expected_aligned(c) if kernel in NATIVE_FORWARD else None, pcm_taken(c)]
