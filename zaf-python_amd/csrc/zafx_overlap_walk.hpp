// zafx_overlap_walk.hpp -- what the fused STFT-mask-ISTFT kernels share: k_center (zafx_center.hip), k_maskfilter (zafx_maskfilter.hip) and
// k_maskfilter_stems (zafx_maskfilter_stems.hip).  Three translation units, one walk:
//
// the deal of units to workgroups (deal_rounds, deal_unit), an equal-length unit's clip and blocks (equal_unit), the read of a RAGGED unit's
// record (read_unit), and on the host the workgroup slots (lds_slots), the window-length dispatch (dispatch_log2w) and the launch (launch_walk).
//
// Every device piece is forced inline and compiles to the very instructions it had when each kernel carried a copy of it: the kernels' code
// objects are held to that, and that bar decides what is here and how it is written (DESIGN.md 4.13 "Code objects").  equal_unit returns its
// blocks by value (through references k_center's schedule changed), and the deal's backward step is written once per counter width: k_center
// counts its units in 64 bits, the mask-filter kernels' RAGGED forms in 32 (zafx_maskfilter.hip says why).  The mask load, the tile's
// overlap-add and the guarded stores of the two mask-filter kernels moved registers or instructions in every form tried as a function:
// each of the two kernels keeps its copy of them.
#pragma once
#include <algorithm>
#include <type_traits>

#include "zafx_internal.hpp"

namespace zafx {

// ---- the deal.  Equal-length: position w of the walk is unit w.  RAGGED: the units come ordered by descending length, and the rounds of
// gridDim.x units are dealt forwards and backwards in turn -- the workgroup that took the longest unit of one round takes the shortest of the
// next (still a fixed deal: nothing is claimed).  The walk runs over whole rounds (deal_rounds); the last one may be short.
template <bool RAGGED, class Cnt>
__device__ __forceinline__ Cnt deal_rounds(Cnt n_units) {
    return RAGGED ? (n_units + gridDim.x - 1) / gridDim.x * gridDim.x : n_units;
}

// The unit of position w = blockIdx.x + round * gridDim.x; false: the position holds none (the last round may be short; uniform).
// A backward round's unit is (2 round + 1) gridDim.x - 1 - w = (round + 1) gridDim.x - 1 - blockIdx.x: 64-bit counters take it from w, 32-bit
// ones from blockIdx.x -- the form each kernel was measured with.
template <bool RAGGED, class Cnt, class Round>
__device__ __forceinline__ bool deal_unit(Cnt w, Round round, Cnt n_units, Cnt& u) {
    u = w;
    if constexpr (RAGGED) {
        if constexpr (sizeof(Cnt) == 8) {
            if (round & 1) u = (2LL * round + 1) * gridDim.x - 1 - w;
        } else {
            if (round & 1) u = (round + 1) * gridDim.x - 1 - blockIdx.x;
        }
        if (u >= n_units) return false;
    }
    return true;
}

// Equal-length batches: unit u = clip * n_segs + seg is blocks [b0, b1) = [seg * seg_blocks, min(n_blocks, (seg + 1) * seg_blocks)) of its clip.
struct EqualUnit { long long clip; int b0, b1; };
__device__ __forceinline__ EqualUnit equal_unit(long long u, int n_segs, int seg_blocks, int n_blocks) {
    const long long clip = u / n_segs;
    const int seg = (int)(u - clip * n_segs);
    const int b0 = seg * seg_blocks;
    return {clip, b0, min(n_blocks, b0 + seg_blocks)};
}

// RAGGED: record u of the device table (CenterUnit / MaskfilterUnit, zafx_units.hpp), uniform: read with scalar loads.
template <class Unit, class Cnt>
__device__ __forceinline__ Unit read_unit(const Unit* __restrict__ table, Cnt u) {
    return table[__builtin_amdgcn_readfirstlane((int)u)];   // (the launcher keeps the units below 2^31)
}

// ---- the host side of the launchers.

// workgroups the device holds at once: what LDS admits per CU, at most 4
inline long long lds_slots(int n_cus, size_t smem_bytes) {
    return (long long)n_cus * (int)std::max<size_t>(1, std::min<size_t>(4, (size_t)kMaxLdsBytes / smem_bytes));
}

// fn(std::integral_constant<int, LOG2W>{}) for a window length W = 2^log2w of 256 .. 2048; false, and fn not called, for any other.
template <class Fn>
bool dispatch_log2w(int log2w, Fn fn) {
    switch (log2w) {
        case 8: fn(std::integral_constant<int, 8>{}); return true;
        case 9: fn(std::integral_constant<int, 9>{}); return true;
        case 10: fn(std::integral_constant<int, 10>{}); return true;
        case 11: fn(std::integral_constant<int, 11>{}); return true;
    }
    return false;
}

// One launch of a walk kernel of W = 2^LOG2W: `units` units over at most `slots` workgroups of nt threads, the kernel's arguments args...
// followed by the unit count and the gain 1 / (W cola_gain) (ifft's 1 / W, then zaf.py:241).  `name` is what the plan reports as run, with or
// without units.
template <int LOG2W, class Kern, class... Args>
hipError_t launch_walk(const zafx_plan& pl, Kern kern, const char* name, int nt, size_t smem, long long units, long long slots, const Args&... args) {
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), pl.device, smem); e != hipSuccess) return e;
    pl.ran = name;
    if (units <= 0) return hipSuccess;
    const float gain = 1.f / ((float)(1 << LOG2W) * pl.cola_gain);
    hipLaunchKernelGGL(kern, dim3((unsigned)std::min(units, slots)), dim3(nt), smem, pl.stream, args..., units, gain);
    return hipGetLastError();
}

}  // namespace zafx
