// solvempc_amd/csrc/mpcq_lane.h — the cross-lane and typed scalar primitives every kernel file shares: DPP moves,
// readlane, the permlane self-swap, the reductions and 32-lane scans built on them, OSQP's limit_scaling and the
// typed fma / abs / max / min.  Nothing here knows a kernel's data layout.
//
// THE EXEC-MASK CONTRACT.  The DPP moves run with bound_ctrl: a lane without a source lane (a row shift's
// first lanes) and a lane whose source lane is inactive both read 0.  readlane and the permlane swaps read
// whatever an inactive lane's register holds.  So the moves, and every reduction and scan below, are only
// correct under a full EXEC mask: call them in wave-uniform control flow, all 64 lanes active, with dead
// lanes masked by value (the op's identity) and never by a branch.
#pragma once
#include "mpcq_internal.h"

namespace mpcq {

// ---- typed scalars
template <typename T> __device__ __forceinline__ T tt_fma(T a, T b, T c);
template <> __device__ __forceinline__ float tt_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <> __device__ __forceinline__ double tt_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename T> __device__ __forceinline__ T tt_abs(T a) { return a < T(0) ? -a : a; }
template <typename T> __device__ __forceinline__ T tt_max(T a, T b) { return a > b ? a : b; }
template <typename T> __device__ __forceinline__ T tt_min(T a, T b) { return a < b ? a : b; }
// IEEE minNum / maxNum / |x| at the operand's own width (__builtin_fmin & co. are the double builtins:
// on float operands they widen, compare in fp64 and narrow back)
__device__ __forceinline__ float tt_fmin(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double tt_fmin(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ float tt_fmax(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double tt_fmax(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ float tt_fabs(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ double tt_fabs(double a) { return __builtin_fabs(a); }

// OSQP scaling.c limit_scaling: a norm below MIN_SCALING counts as 1, one above MAX_SCALING is clipped
__device__ inline double limit_scaling(double d)
{
    d = d < kMinScaling ? 1.0 : d;
    return d > kMaxScaling ? kMaxScaling : d;
}

__device__ __forceinline__ bool wave_any(bool p) { return __ballot(p) != 0ull; }
__device__ __forceinline__ bool wave_all(bool p) { return __ballot(!p) == 0ull; }

// ---- moves
// DPP move; a lane without a source, or in a row outside the row mask RM, reads 0.  With every row enabled the
// zero comes from bound_ctrl: no "old" operand, so no copy (or zeroing) of the destination before the move.
template <int CTRL, int RM = 0xF> __device__ __forceinline__ unsigned dpp_u(unsigned v)
{
    if constexpr (RM == 0xF) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
    else return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, RM, 0xF, false);
}
template <int CTRL, int RM = 0xF> __device__ __forceinline__ float dpp_t(float v)
{
    return __uint_as_float(dpp_u<CTRL, RM>(__float_as_uint(v)));
}
template <int CTRL, int RM = 0xF> __device__ __forceinline__ double dpp_t(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = dpp_u<CTRL, RM>((unsigned)u), hi = dpp_u<CTRL, RM>((unsigned)(u >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ float readlane_t(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double readlane_t(double v, int l)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// op(own value, partner's value) across the gfx950 lane swaps (VALU, no LDS round trip).  W = 16:
// v_permlane16_swap, 16-lane rows 0 <-> 1 and 2 <-> 3; W = 32: v_permlane32_swap, lanes 0-31 <-> 32-63.  After
// a swap of v with itself {r[0], r[1]} = {own, partner} in some order, so a symmetric op gives both partners
// the same bits.
template <int W> __device__ __forceinline__ auto self_swap(unsigned v)
{
    static_assert(W == 16 || W == 32, "permlane16 or permlane32");
    if constexpr (W == 16) return __builtin_amdgcn_permlane16_swap(v, v, false, false);
    else return __builtin_amdgcn_permlane32_swap(v, v, false, false);
}
template <int W, typename F> __device__ __forceinline__ unsigned swap_op(unsigned v, F op)
{
    auto r = self_swap<W>(v);
    return op(r[0], r[1]);
}
template <int W, typename F> __device__ __forceinline__ float swap_op(float v, F op)
{
    auto r = self_swap<W>(__float_as_uint(v));
    return op(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
template <int W, typename F> __device__ __forceinline__ double swap_op(double v, F op)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    auto r = self_swap<W>((unsigned)u);
    auto h = self_swap<W>((unsigned)(u >> 32));
    auto mk = [](unsigned l, unsigned hh) { return __longlong_as_double((long long)(((unsigned long long)hh << 32) | l)); };
    return op(mk(r[0], h[0]), mk(r[1], h[1]));
}

// ---- reductions with a symmetric op, every lane of the reduced set ending on the same bits.  One association
// order: quad swaps, half-row and row mirrors (DPP), then the 16-lane swap (a 32-lane half) and the 32-lane
// swap (the wave).  (A __shfl_xor butterfly associates differently and gives other bits: those keep their
// own names where they live.)
template <typename T, typename F> __device__ __forceinline__ T half_reduce(T v, F op)
{
    v = op(v, dpp_t<0xB1>(v));   // quad_perm [1,0,3,2]
    v = op(v, dpp_t<0x4E>(v));   // quad_perm [2,3,0,1]
    v = op(v, dpp_t<0x141>(v));  // row_half_mirror
    v = op(v, dpp_t<0x140>(v));  // row_mirror
    return swap_op<16>(v, op);   // never across the halves
}
template <typename T, typename F> __device__ __forceinline__ T wave_reduce(T v, F op)
{
    return swap_op<32>(half_reduce(v, op), op);
}

// ---- inclusive scans, op with identity 0 (sums, maxima of non-negative values).  row_prefix / row_suffix
// scan inside each 16-lane row (row_shr / row_shl 1, 2, 4, 8: the first / last lanes read 0); lane_prefix /
// lane_suffix carry once across rows 0 and 1 for a scan over lanes 0..31 (lanes 32..63 take part in the row
// steps only; for the suffix, lanes past the data must hold 0).
template <typename T, typename F> __device__ __forceinline__ T row_prefix(T v, F op)
{
    v = op(v, dpp_t<0x111>(v));
    v = op(v, dpp_t<0x112>(v));
    v = op(v, dpp_t<0x114>(v));
    return op(v, dpp_t<0x118>(v));
}
template <typename T, typename F> __device__ __forceinline__ T row_suffix(T v, F op)
{
    v = op(v, dpp_t<0x101>(v));
    v = op(v, dpp_t<0x102>(v));
    v = op(v, dpp_t<0x104>(v));
    return op(v, dpp_t<0x108>(v));
}
template <typename T, typename F> __device__ __forceinline__ T lane_prefix(T v, F op, int lane)
{
    v = row_prefix(v, op);
    const T s = readlane_t(v, 15);  // row 0's total
    return (lane >= 16) ? op(v, s) : v;
}
template <typename T, typename F> __device__ __forceinline__ T lane_suffix(T v, F op, int lane)
{
    v = row_suffix(v, op);
    const T s = readlane_t(v, 16);  // row 1's total
    return (lane < 16) ? op(v, s) : v;
}

}  // namespace mpcq
