// ndt_rstree.h — the schedule of the in-wave reduce-scatter of the pass kernels' 22 split sums (block_reduce_store_split,
// ndt_device.h), written once over an exchange policy X: on the device X moves registers between lanes, on the host
// (tests/native/reduce_tree_check.cpp) it holds a whole wave per value.  No device header is needed to read it.
//
// Every lane carries 22 sums; lanes 0-31 and 32-63 of a wave carry different sets (the pair loop already added across
// lane bit 32).  The sums are added across lane bits 16, 8, 4, 2, 1: at each step a lane keeps half of what it carries
// and adds its partner's copy of that half.  22 -> 11 -> 6 -> 3 -> 2 -> 1 slots: 11 + 6 + 3 + 2 + 1 = 23 exchanges.  An
// odd slot count leaves one slot without a slot to trade against: both lanes keep it and add the partner's copy (`both`).
//
// The sum of one value is a fixed tree of IEEE additions: x[l] + x[partner(l)] at every step, the partner being l ^ 16,
// l ^ 8, l ^ 7 (row_half_mirror: the lane bit 4 step pairs lanes 0-7, 1-6, 2-5, 3-4 of every eight), l ^ 2, l ^ 1.
// Which of two partners keeps a value changes no bit: additions commute, and the eight lanes' mirror pairing hands the
// same four pair sums to the next step whichever half keeps them.  So the tree is that of the schedule this one
// replaced (32 slots, ten of them zeros, 31 exchanges); the host check compares the two bit for bit.
#pragma once

#ifndef __host__  // a host compiler
#define __host__
#define __device__
#endif

namespace ndt {

constexpr int kRsValues = 22;

// X::T a value (one lane's on the device, a wave's on the host);
// X::swap16(A, B): lanes with bit 16 clear get A + partner's A, the others B + partner's B;
// X::xchg<M>(A, B): lanes with bit M clear keep A and add the partner's A (which the partner does not keep), lanes with
//                   bit M set keep B and add the partner's B;
// X::both<M>(A):    every lane gets A + partner's A.
template <class X>
__host__ __device__ inline typename X::T rs22_reduce(const X& x, const typename X::T (&v)[kRsValues]) {
    typename X::T a1[11], a2[6], a3[3], a4[2];
    for (int i = 0; i < 11; ++i) a1[i] = x.swap16(v[i], v[i + 11]);
    for (int j = 0; j < 5; ++j) a2[j] = x.template xchg<8>(a1[2 * j], a1[2 * j + 1]);
    a2[5] = x.template both<8>(a1[10]);
    for (int j = 0; j < 3; ++j) a3[j] = x.template xchg<4>(a2[j], a2[j + 3]);
    a4[0] = x.template xchg<2>(a3[0], a3[2]);
    a4[1] = x.template both<2>(a3[1]);
    return x.template xchg<1>(a4[0], a4[1]);
}

// The value (0..21) whose wave total rs22_reduce leaves in `lane` (of either half-wave)
__host__ __device__ constexpr int rs22_value(int lane) {
    const int j3 = (lane & 1) ? 1 : ((lane & 2) ? 2 : 0);  // slot of the lane bit 2 step's input
    const int j2 = j3 + ((lane & 4) ? 3 : 0);              // ... of the lane bit 4 step's
    const int i = j2 == 5 ? 10 : 2 * j2 + ((lane & 8) ? 1 : 0);
    return i + ((lane & 16) ? 11 : 0);
}
// Two lanes hold the same total where a `both` step left it on both sides: the one with that lane bit clear reports it
__host__ __device__ constexpr bool rs22_reports(int lane) {
    const int j3 = (lane & 1) ? 1 : ((lane & 2) ? 2 : 0);
    const int j2 = j3 + ((lane & 4) ? 3 : 0);
    return !(j3 == 1 && (lane & 2)) && !(j2 == 5 && (lane & 8));
}

}  // namespace ndt
