"""zaf-python_amd/csrc/zafx_routes.hpp -- the one place an equal-length float32 call's kernel is decided -- on the CPU: the header compiled by
g++ into tests/host_emu/routes_emu.cpp (once more under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program) and held to

* every record of long_clips.BOUNDS: the kernel below and above the bound, the form flags where the name stays, and cond(n) on the eight
  lengths of the route on either side;
* the bounds on n_clips x tiles that no batch a device holds reaches: the route flips to the launcher's fallback exactly at the bound;
* sharing: the fused-mel predicate at W = 4096 against the STFT band route, the three int16 predicates against the float route's `aligned`;
* the kernels recorded on the GPU (tests/golden/call_routes.json) for the calls of tests/route_cases.py;
* the ragged entry points: the kernels and flags recorded on the GPU (tests/golden/ragged_routes.json) for the batches of
  tests/ragged_route_cases.py, every bound on a clip, a block, a tile count and an address from both sides, and the conditions the ragged plan
  predicates share with the equal-length routes.
No GPU, nothing allocated."""
import json
import os
import subprocess

import numpy as np
import pytest

import long_clips as lc
import ragged_route_cases as rr
import route_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_emu", "routes_emu.cpp")
INC = os.path.join(ROOT, "zaf-python_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "call_routes.json")
RAGGED_GOLDEN = os.path.join(ROOT, "tests", "golden", "ragged_routes.json")


def _runner(exe):
    def run(lines):
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout[-500:] + res.stderr[-2000:]
        out = [dict(f.split("=") for f in ln.split()) for ln in res.stdout.strip().split("\n")]
        assert len(out) == len(lines)
        return out
    return run


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("routes") / "routes_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", INC, SRC, "-o", str(exe)], check=True)
    return _runner(exe)


@pytest.fixture(scope="module")
def emu_sanitized(tmp_path_factory):
    """The same stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, run directly."""
    exe = tmp_path_factory.mktemp("routes_san") / "routes_emu_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", INC, SRC, "-o", str(exe)], check=True)
    return _runner(exe)


# ------------------------------------------------------------------------------------------------------------ the BOUNDS records
FAMILY = {"stft": ("stft", False), "stft_one_sided": ("stft", True), "magnitude": ("stft", "magnitude"), "power": ("stft", "power"),
          "istft": ("istft", False), "istft_one_sided": ("istft", True), "mdct": ("mdct", False), "imdct": ("imdct", False),
          "mel": ("mel", False), "mfcc": ("mfcc", False), "mel_mfcc": ("mfcc", False), "cqt": ("cqt", False), "chroma": ("chroma", False),
          "center": ("center", False)}


def bound_case(b):
    family, spectrum = FAMILY[b["kind"]]
    o = b["options"]
    return rc.case(family, b["W"] or 65536, b["hop"], spectrum, layout=b["layout"], row_align=o.get("row_align", 0),
                   filters=128 if family in ("mel", "mfcc") else 0, ncoef=20 if family == "mfcc" else 0, pcm=bool(o.get("pcm")))


def bound_line(b, n):
    """The record's call at length n: one clip, both arrays on 256 bytes."""
    c = bound_case(b)
    if c["family"] in ("cqt", "chroma", "center"):
        t = 0
    else:
        t = lc.frames_of(b["kind"] if not rc.is_inverse(c) else {"istft": "stft", "imdct": "mdct"}[c["family"]], n,
                         w=np.zeros(b["W"]), hop=b["hop"])
    return rc.call_line(c, n_clips=1, n=n, frames=t, in_addr=256, out_addr=256)


FLAGS = ("aligned", "vec", "claimed", "carry", "pcm_direct")
# the one record whose condition is the kernel's own (k_imdct's 16-byte gather, device code): the header routes both sides to k_imdct
KERNELS_OWN = ("imdct_2048",)


def on_route_near(b, n, step, count=8):
    out = []
    while len(out) < count:
        if b["on_route"](n):
            out.append(n)
        n += step
    return out


@pytest.mark.parametrize("name", lc.BOUND_NAMES)
def test_every_bound_record_is_the_headers_answer(emu, name):
    b = lc.bound(name)
    below, above = emu([bound_line(b, b["n_below"]), bound_line(b, b["n_above"])])
    print(name, below, above)
    assert below["kernel"] == b["kernel_below"]
    assert above["kernel"] == b["above"]
    if name in KERNELS_OWN:
        assert b["source"].endswith(":k_imdct") and below == above
        return
    # what tells the two sides apart: the kernel, or -- one kernel name on both sides -- the form flags (a flag may also follow the length's
    # parity from one side to the other: only the name is read where it differs)
    differ = ["kernel"] if below["kernel"] != above["kernel"] else [k for k in FLAGS if below[k] != above[k]]
    assert differ, "one kernel name on both sides: the form must differ"
    if b["options"].get("pcm"):
        assert (below["pcm_direct"], above["pcm_direct"]) == ("1", "0")
    lengths = on_route_near(b, b["n_below"], -1) + on_route_near(b, b["n_above"], 1)
    for n, got in zip(lengths, emu([bound_line(b, n) for n in lengths])):
        takes = all(got[k] == below[k] for k in differ)
        assert takes == bool(b["cond"](n)), (n, got)
        assert takes or all(got[k] == above[k] for k in differ), (n, got)


def test_the_records_name_functions_of_the_header():
    text = open(os.path.join(INC, "zafx_routes.hpp")).read()
    for b in lc.BOUNDS:
        file, _, fn = b["source"].partition(":")
        if b["name"] in KERNELS_OWN:
            continue
        assert file == "zafx_routes.hpp" and f" {fn}(" in text, b["source"]


# ------------------------------------------------------------------------------------------------------------ bounds no GPU run reaches
def ceil_div(a, b):
    return -(-a // b)


# (name, the case -- its `frames` the T --, what the bound counts per clip, the bound, the route below it, the route at it).  The fallbacks are the
# launchers' own: a W = 4096 / 8192 call the tiled kernels cannot count runs the one-workgroup-per-tile kernel, k_stft_ft16c's calls run
# k_stft_ft16, k_mel2's |X| runs k_stft_ft16, k_mdct_ft32bc's run k_mdct_ft32b, the fused mel runs the spectrum kernel + k_melfb.
# k_stft_ft16bc's 2^30 tiles sit behind its own n_clips T < 2^31 from T = 2 on (ceil(T / 16) <= T / 2), so that bound is met at T = 1;
# k_mdct_ft32bc's 2^30 units sit behind its 2^40 elements at every T (pitch >= T >= tiles), so that one has no row.
COUNT_BOUNDS = [
    ("stft_band_carry_tiles", rc.case("stft", 4096, 2048, frames=1), lambda t: ceil_div(t, 16), 1 << 30, ("band-carry", "k_stft_ft16bc"), ("generic", "k_stft")),
    ("stft_band_carry_rows", rc.case("stft", 4096, 2048, frames=300), lambda t: t, 1 << 31, ("band-carry", "k_stft_ft16bc"), ("generic", "k_stft")),
    ("stft_band_tiles", rc.case("stft", 4096, 2048, "magnitude", frames=300), lambda t: ceil_div(t, 16), 1 << 31, ("band", "k_stft_ft16b"), ("generic", "k_stft")),
    ("stft_quad_tiles", rc.case("stft", 8192, 4096, "magnitude", frames=300), lambda t: ceil_div(t, 16), 1 << 31, ("quad", "k_stft_ft16q"), ("generic", "k_stft")),
    ("stft_fat_carry_rows", rc.case("stft", 2048, 1024, frames=300), lambda t: t, 1 << 31, ("fat-carry", "k_stft_ft16c"), ("fat", "k_stft_ft16")),
    ("stft_spec2_tiles", rc.case("stft", 2048, 1024, "power", frames=300), lambda t: ceil_div(t, 16), 1 << 31, ("spec2", "k_mel2"), ("fat", "k_stft_ft16")),
    ("istft_duo_units", rc.case("istft", 4096, 2048, frames=300), lambda t: ceil_div(t, 16) + 1, 1 << 30, ("duo", "k_istft_ft16d"), ("generic", "k_istft")),
    ("istft_band_units", rc.case("istft", 4096, 1024, frames=300), lambda t: 2 * ceil_div(t, 16), 1 << 30, ("band", "k_istft_ft16b"), ("generic", "k_istft")),
    ("istft_quad_units", rc.case("istft", 8192, 4096, frames=300), lambda t: ceil_div(t, 8) + 1, 1 << 30, ("quad", "k_istft_ft8q"), ("generic", "k_istft")),
    ("mdct_band_carry_elements", rc.case("mdct", 4096, frames=300), lambda t: 2048 * t, 1 << 40, ("band-carry", "k_mdct_ft32bc"), ("band", "k_mdct_ft32b")),
    ("mdct_band_tiles", rc.case("mdct", 4096, frames=320), lambda t: ceil_div(t, 32), 1 << 31, ("band", "k_mdct_ft32b"), ("generic", "k_mdct")),
    ("mdct_quad_tiles", rc.case("mdct", 8192, frames=300), lambda t: ceil_div(t, 32), 1 << 31, ("quad", "k_mdct_ft32q"), ("generic", "k_mdct")),
    ("imdct_quad_units", rc.case("imdct", 8192, frames=300), lambda t: ceil_div(t, 16) + 1, 1 << 30, ("quad", "k_imdct_q"), ("generic", "k_imdct")),
    ("mel_band_tiles", rc.case("mel", 4096, 2048, filters=128, frames=300), lambda t: ceil_div(t, 16), 1 << 31, ("band", "k_mel_ft16b"), ("wide", "k_melfb")),
]


@pytest.mark.parametrize("name,c,per_clip,limit,below,at", COUNT_BOUNDS, ids=[b[0] for b in COUNT_BOUNDS])
def test_count_bounds_flip_to_the_fallback(emu, name, c, per_clip, limit, below, at):
    t = c["frames"]
    n_at = ceil_div(limit, per_clip(t))            # the first clip count at which  n_clips x per_clip < limit  fails
    assert (n_at - 1) * per_clip(t) < limit <= n_at * per_clip(t)
    got = emu([rc.call_line(c, n_clips=n_at - 1), rc.call_line(c, n_clips=n_at)])
    print(name, n_at, got)
    assert [(g["route"], g["kernel"]) for g in got] == [below, at]


def test_mdct_carry_form_stops_at_its_tile_count(emu):
    """k_mdct_ft32's carry instantiation counts tiles in 32 bits: the same kernel name either side, the carry flag flips."""
    c = rc.case("mdct", 2048, frames=300)
    n_at = ceil_div(1 << 31, ceil_div(300, 32))
    below, at = emu([rc.call_line(c, n_clips=n_at - 1), rc.call_line(c, n_clips=n_at)])
    assert (below["kernel"], below["carry"], at["kernel"], at["carry"]) == ("k_mdct_ft32", "1", "k_mdct_ft32", "0")
    assert below["aligned"] == at["aligned"] == "1"


# ------------------------------------------------------------------------------------------------------------ sharing
def _draws(seed, count):
    """Calls that straddle every term of the shared conditions: lengths around 2^28 / 2^29, frame counts around 2^29 / H, clip counts around
    2^31 tiles, addresses at every residue of 16."""
    r = np.random.default_rng([47, seed])
    for _ in range(count):
        n = int(r.choice([1 << 20, (1 << 28) - 4, 1 << 28, (1 << 29) - 4, 1 << 29])) + int(r.choice([-4, -2, -1, 0, 0, 1, 2, 4]))
        t = int(r.choice([33, 300, (1 << 18) - 16, (1 << 18) - 15, 1 << 18, 1 << 19])) + int(r.integers(-2, 3))
        clips = int(r.choice([1, 2, 1 << 12, 1 << 13, 1 << 27]))
        yield n, t, clips, 256 + int(r.choice([0, 0, 8, 16, 4, 12, 1, 2, 6]))


def test_fused_mel_and_stft_band_share_their_condition(emu):
    mel = rc.case("mel", 4096, 2048, filters=128)
    mag = rc.case("stft", 4096, 2048, "magnitude")
    draws = list(_draws(1, 400))
    a = emu([rc.call_line(mel, n_clips=k, n=n, frames=t, in_addr=x) for n, t, k, x in draws])
    b = emu([rc.call_line(mag, n_clips=k, n=n, frames=t, in_addr=x) for n, t, k, x in draws])
    usable = [g["band_usable"] == "1" for g in a]
    assert [g["route"] == "band" for g in a] == usable == [g["route"] == "band" for g in b]
    assert 40 < sum(usable) < 360   # (both answers occur)


def test_int16_predicates_agree_with_the_float_routes_aligned_form(emu):
    draws = list(_draws(2, 400))
    stft = rc.case("stft", 2048, 2048, True, pcm=True)
    got = emu([rc.call_line(stft, n_clips=1, n=n, frames=t, in_addr=x) for n, t, _, x in draws])
    for d, g in zip(draws, got):
        if g["pcm_direct"] == "1":
            assert g["route"] in ("fat", "fat-carry") and g["aligned"] == "1" and g["pcm"] == "1", (d, g)
        if g["route"] == "fat-carry":
            assert g["pcm_direct"] == g["aligned"], (d, g)
    assert 20 < sum(g["pcm_direct"] == "1" for g in got) < 380
    mdct = rc.case("mdct", 2048, pcm=True)
    got = emu([rc.call_line(mdct, n_clips=1, n=n, frames=t, in_addr=x) for n, t, _, x in draws])
    for d, g in zip(draws, got):
        assert g["route"] == "persistent" and g["pcm_direct"] == g["aligned"], (d, g)
    assert 10 < sum(g["pcm_direct"] == "1" for g in got) < 390
    mel = rc.case("mel", 2048, 1024, filters=40, pcm=True)
    got = emu([rc.call_line(mel, n_clips=1, n=n, frames=t, in_addr=x) for n, t, _, x in draws])
    for (n, t, _, x), g in zip(draws, got):
        assert g["route"] == "mel2" and (g["pcm_direct"] == "1") == (n < 1 << 29), (n, g)
        assert (g["aligned"] == "1") == (g["pcm_direct"] == "1" and n % 2 == 0 and x % 8 == 0), (n, x, g)


# ------------------------------------------------------------------------------------------------------------ the recorded calls
def test_cases_have_the_frames_they_say():
    for name, c in rc.CASES.items():
        if rc.is_inverse(c):
            continue
        kind = {"stft": "stft", "mdct": "mdct", "mel": "stft", "mfcc": "stft"}[c["family"]]
        assert lc.frames_of(kind, rc.samples(c), w=np.zeros(c["W"]), hop=c["hop"]) == c["frames"] in (rc.ON, rc.OFF), name


def test_the_header_names_the_kernels_the_gpu_ran(emu):
    golden = json.load(open(GOLDEN))
    assert list(golden) == list(rc.CASES)
    names = list(rc.CASES)
    for name, got in zip(names, emu([rc.call_line(rc.CASES[n]) for n in names])):
        c = rc.CASES[name]
        # an int16 call the kernels do not read themselves runs the float route on the plan's staging array (on 256 bytes, the same geometry)
        assert got["kernel"] == golden[name][0], (name, got)
        if c["pcm"]:
            assert (got["pcm_direct"] == "1") == (c["short"] == 0 or c["family"] == "mel" or c["spectrum"] == "magnitude"), (name, got)


def test_sanitized_build_answers_the_same(emu, emu_sanitized):
    lines = [rc.call_line(c) for c in rc.CASES.values()] + [bound_line(b, n) for b in lc.BOUNDS for n in (b["n_below"], b["n_above"])]
    lines += [rr.call_line(c) for c in rr.CASES.values()] + [ln for _, _, sides in RAGGED_BOUNDS for ln, _ in sides]
    assert emu_sanitized(lines) == emu(lines)


# ------------------------------------------------------------------------------------------------------------ the ragged entry points
def test_the_header_names_the_ragged_kernels_the_gpu_ran(emu):
    """Every batch of ragged_route_cases.py: the kernel the GPU ran on the parent, the `aligned` flag its conditions gave the launch, and
    whether its int16 launch took an integer batch."""
    golden = json.load(open(RAGGED_GOLDEN))
    assert list(golden) == list(rr.CASES)
    names = list(rr.CASES)
    got = dict(zip(names, emu([rr.call_line(rr.CASES[n]) for n in names])))
    left = [n for n in names if got[n]["route"] == "pcm-not-taken"]
    as_float = dict(zip(left, emu([rr.call_line(rr.CASES[n], as_float=True) for n in left])))
    for name in names:
        kernel, _, aligned, taken = golden[name]
        g = got[name]
        if taken is not None:
            assert (g["route"] != "pcm-not-taken") == bool(taken), (name, g)
            assert (g["kernel"] == "none") == (not taken), (name, g)
            g = g if taken else as_float[name]   # (the staging array's float batch)
        if kernel.startswith("per-clip ") or (rr.is_inverse(rr.CASES[name]) and not kernel.endswith("_ragged")):
            assert (g["route"], g["kernel"]) == ("per-clip", "per-clip"), (name, g)
        else:
            assert g["kernel"] == kernel and g["route"] != "per-clip", (name, g)
        if aligned is not None:
            assert g["aligned"] == str(aligned), (name, g)
    assert sum(v[3] == 1 for v in golden.values()) >= 8 and sum(v[3] == 0 for v in golden.values()) >= 8


def _one(name, n, **kw):
    """One clip of n samples (its frames follow) of a case's plan, everything else the case's."""
    c = rr.CASES[name]
    t = -(-n // c["hop"]) + 1
    return rr.call_line(c, offsets=[0], lens=[n], frms=[t], **kw)


def _blocks(name, frames):
    return rr.call_line(rr.CASES[name], offsets=[0] * len(frames), lens=frames, frms=frames)


NATIVE = {"mdct": ("mdct-native", "k_mdct_ft32_ragged"), "stft": ("stft-native", "k_stft_ft16_ragged"), "mag": ("stft-native", "k_mel2_ragged"),
          "mel": ("mel-native", "k_mel2_ragged"), "f64": ("f64-native", "k_stft_ft8_f64_ragged"), "imdct": ("native", "k_imdct_ragged"),
          "istft": ("native", "k_istft_ragged")}
PER_CLIP, NOT_TAKEN, TOO_LARGE = ("per-clip", "per-clip"), ("pcm-not-taken", "none"), ("too-large", "refused")
I32 = (1 << 31) - 1
# (name, what the bound counts, [(line, (route, kernel)) below the bound, the same at it]).  Arithmetic only: no device holds these batches.
RAGGED_BOUNDS = [
    ("mdct_2_28_samples", "a clip's samples", [(_one("mdct_2048", (1 << 28) - 4), NATIVE["mdct"]), (_one("mdct_2048", 1 << 28), PER_CLIP)]),
    ("mdct_int16_2_28_frames", "a clip's sample frames", [(_one("pcm_mdct_c1", (1 << 28) - 4), NATIVE["mdct"]), (_one("pcm_mdct_c1", 1 << 28), NOT_TAKEN)]),
    ("spec2_2_29_samples", "a clip's samples", [(_one("stft_2048_mag", (1 << 29) - 2), NATIVE["mag"]), (_one("stft_2048_mag", 1 << 29), PER_CLIP)]),
    ("mel_2_29_samples", "a clip's samples", [(_one("mel_2048", (1 << 29) - 2), NATIVE["mel"]), (_one("mel_2048", 1 << 29), PER_CLIP)]),
    ("stft_int16_2_29_frames", "a clip's sample frames", [(_one("pcm_stft_one_c1", (1 << 29) - 2), NATIVE["stft"]), (_one("pcm_stft_one_c1", 1 << 29), NOT_TAKEN)]),
    # the complex STFT of float samples has no bound on the clip: the same length stays native
    ("stft_float_unbounded", "nothing", [(_one("stft_2048_two", (1 << 29) - 2), NATIVE["stft"]), (_one("stft_2048_two", 1 << 29), NATIVE["stft"])]),
    # the call's own bound: 2^31 tiles of 16 frames, counted on the frame counts themselves -- one clip reaches it (its pitch is past 2^31:
    # below the bound it runs per clip)
    ("call_2_31_tiles16", "16-frame tiles", [(rr.call_line(rr.CASES["mdct_2048"], offsets=[0], lens=[0], frms=[16 * I32]), PER_CLIP),
                                             (rr.call_line(rr.CASES["mdct_2048"], offsets=[0], lens=[0], frms=[16 * I32 + 1]), TOO_LARGE)]),
    # 2^31 tiles of 8 frames (k_stft_ft8_f64): a pitch below 2^31 - 1 allows 2^31 - 8 frames, 2^28 - 1 tiles, a clip -- eight such clips and
    # eight tiles more (57 frames: a tile is counted from its first frame) reach the bound, and stay below the call's
    ("f64_stft_2_31_tiles8", "8-frame tiles", [(rr.call_line(rr.CASES["f64_stft_two"], offsets=[0] * 9, lens=[0] * 9, frms=[(1 << 31) - 8] * 8 + [56]), NATIVE["f64"]),
                                               (rr.call_line(rr.CASES["f64_stft_two"], offsets=[0] * 9, lens=[0] * 9, frms=[(1 << 31) - 8] * 8 + [57]), PER_CLIP)]),
    ("imdct_block_2_32_bytes", "(W / 2) x pitch x 4", [(_blocks("imdct_2048", [(1 << 20) - 4]), NATIVE["imdct"]), (_blocks("imdct_2048", [1 << 20]), PER_CLIP)]),
    ("imdct_second_block", "(W / 2) x pitch x 4", [(_blocks("imdct_2048", [33, (1 << 20) - 4]), NATIVE["imdct"]), (_blocks("imdct_2048", [33, 1 << 20]), PER_CLIP)]),
    ("istft_block_2_31_bytes", "W x pitch x 8", [(_blocks("istft_2048_two", [(1 << 17) - 4]), NATIVE["istft"]), (_blocks("istft_2048_two", [1 << 17]), PER_CLIP)]),
    ("istft_256_block_2_31_bytes", "W x pitch x 8", [(_blocks("istft_256", [33, (1 << 20) - 4]), NATIVE["istft"]), (_blocks("istft_256", [33, 1 << 20]), PER_CLIP)]),
    ("imdct_base_on_4_bytes", "d_coefs", [(rr.call_line(rr.CASES["imdct_2048"], in_addr=260), NATIVE["imdct"]), (rr.call_line(rr.CASES["imdct_2048"], in_addr=258), PER_CLIP)]),
    ("istft_base_on_4_bytes", "d_spec", [(rr.call_line(rr.CASES["istft_2048_two"], in_addr=260), NATIVE["istft"]), (rr.call_line(rr.CASES["istft_2048_two"], in_addr=258), PER_CLIP)]),
    ("mdct_base_on_4_bytes", "d_in", [(rr.call_line(rr.CASES["mdct_2048"], in_addr=260), NATIVE["mdct"]), (rr.call_line(rr.CASES["mdct_2048"], in_addr=258), PER_CLIP)]),
]


@pytest.mark.parametrize("name,counts,sides", RAGGED_BOUNDS, ids=[b[0] for b in RAGGED_BOUNDS])
def test_ragged_bounds_from_both_sides(emu, name, counts, sides):
    got = emu([ln for ln, _ in sides])
    print(name, counts, got)
    assert [(g["route"], g["kernel"]) for g in got] == [want for _, want in sides]


def test_ragged_grids_from_both_sides(emu):
    """The grids that do not move a bound: rows of whole 128-byte lines (64-byte rows stay per clip), offsets and lengths on the 2-sample
    grid of `aligned` (2 mod 4 is even), k_stft_ft16's radix-32 twiddles at W = 2048."""
    c = rr.CASES["stft_2048_two"]
    half, whole = emu([rr.call_line(dict(c, row_align=8)), rr.call_line(c)])   # pitches 8, 8, 40 against 16, 16, 48 complex64
    assert (half["route"], whole["route"]) == ("per-clip", "stft-native")
    offs, lens = rr.in_offsets(c), rr.lengths(c)
    for line in (rr.call_line(c, offsets=[offs[0], offs[1] + 2, offs[2]]), rr.call_line(c, lens=[lens[0], lens[1] + 2, lens[2] - 2])):
        got = emu([line])[0]
        assert (got["kernel"], got["aligned"]) == ("k_stft_ft16_ragged", "1"), got
    for name, want in (("stft_2048_two", "per-clip"), ("stft_2048_one", "per-clip"), ("stft_2048_mag", "stft-native"), ("stft_1024_two", "stft-native")):
        assert emu([rr.call_line(rr.CASES[name], tw_r32=0)])[0]["route"] == want, name


def test_ragged_tile_bounds_behind_the_calls_own(emu):
    """tiles32 < 2^31 (k_mdct_ft32) and tiles16 < 2^31 (the float64 MDCT and mel) repeat the call's bound on 16-frame tiles and never decide: the
    largest batch the call takes -- clips of the most frames a pitch below 2^31 - 1 allows, the last one cut to 2^31 - 1 tiles of 16 in all --
    is native, with half as many tiles of 32; one more frame and the call itself is refused.  frames < 2^28 of the ISTFT's blocks sits behind
    its byte bound the same way: W x pitch x 8 < 2^31 allows no block of 2^28 frames at any W."""
    for name, want in (("mdct_2048", NATIVE["mdct"]), ("f64_mdct", ("f64-native", "k_mdct_ft16_f64_ragged")), ("f64_mel", ("f64-native", "k_mel_ft8_f64_ragged"))):
        c = rr.CASES[name]
        most = (1 << 31) - c["row_align"]
        per = ceil_div(most, 16)
        whole, rest = divmod(I32, per)
        assert rest > 0
        below, at = [most] * whole + [16 * rest], [most] * whole + [16 * rest + 1]
        assert sum(ceil_div(t, 16) for t in below) == I32 and sum(ceil_div(t, 32) for t in below) < 1 << 31
        below, at = emu([rr.call_line(c, offsets=[0] * len(f), lens=[0] * len(f), frms=f) for f in (below, at)])
        assert (below["route"], below["kernel"]) == want and (at["route"], at["kernel"]) == TOO_LARGE, (name, below, at)
    for w in (256, 512, 1024, 2048):
        assert w * (1 << 28) * 8 >= 1 << 31
    got = emu([_blocks("istft_256", [(1 << 28) - 4]), _blocks("istft_256", [1 << 28])])
    assert [(g["route"], g["kernel"]) for g in got] == [PER_CLIP, PER_CLIP]


def test_ragged_stft_plans_are_the_fat_kernels_with_their_tables(emu):
    """stft_ragged_native = stft_use_fat (W = 256 ... 2048, reference layout) + the twiddle tables; |X| / |X|^2 at W = 2048 go to k_mel2."""
    base = rr.CASES["stft_2048_two"]
    for w in (64, 128, 256, 512, 1024, 2048, 4096, 8192):
        for layout in ("FT", "TF"):
            for spec in (False, True, "magnitude", "power"):
                c = dict(base, W=w, hop=w // 2, layout=layout, spectrum=spec, row_align=rr.case("stft", w, w // 2, spec, layout=layout)["row_align"])
                equal = emu([rc.call_line(rc.case("stft", w, w // 2, spec, layout=layout, row_align=16), n_clips=1, n=32 * (w // 2), frames=33)])[0]
                with_tables, without = emu([rr.call_line(c), rr.call_line(c, tables=0)])
                fat = layout == "FT" and 256 <= w <= 2048
                assert (with_tables["route"] == "stft-native") == fat, (w, layout, spec, with_tables)
                assert without["route"] == "per-clip", (w, layout, spec, without)
                if fat:   # the family the equal-length route runs the same plan on (k_mel2 takes the real kinds at W = 2048 in both)
                    assert equal["route"] in ("fat", "fat-carry", "spec2"), equal
                    assert (with_tables["kernel"] == "k_mel2_ragged") == (equal["route"] == "spec2") == (w == 2048 and spec in ("magnitude", "power"))


def test_ragged_spec2_implies_the_equal_length_route_on_each_clip(emu):
    """A batch of |X| / |X|^2 clips that runs on k_mel2's RAGGED form: every clip alone, as an equal-length call, takes k_mel2 too."""
    r = np.random.default_rng([47, 3])
    c = rr.CASES["stft_2048_mag"]
    taken = 0
    for _ in range(60):
        lens = [int(r.choice([0, 1024, 1 << 20, (1 << 29) - 2, (1 << 29) - 1, 1 << 29])) for _ in range(3)]
        frms = [-(-n // 1024) + 1 for n in lens]
        batch = emu([rr.call_line(c, offsets=[0, 0, 0], lens=lens, frms=frms)])[0]
        if batch["kernel"] != "k_mel2_ragged":
            assert max(lens) >= 1 << 29 and batch["route"] == "per-clip", (lens, batch)
            continue
        taken += 1
        eq = rc.case("stft", 2048, 1024, "magnitude", row_align=32)
        for g in emu([rc.call_line(eq, n_clips=1, n=n, frames=t) for n, t in zip(lens, frms)]):
            assert (g["route"], g["kernel"]) == ("spec2", "k_mel2"), (lens, g)
    assert 5 < taken < 55
