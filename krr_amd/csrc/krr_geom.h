// krr_geom.h — how one wave streams values[beg, end): the layout every streaming loop
// (stream_segment, kll_stream, the KLL tail-lines pass) and every chunk processor that needs
// positions share.  Host + device, integers only; compiles under plain g++ (tests/native).
//
// THE CONTRACT.  A segment is L = end - beg slots; slot i is values[beg + i].  values is 16-byte
// aligned, so the slots from a0 = beg rounded up to even, up to a1 = end rounded down to even,
// form nunits double2 units: the body.  An odd beg leaves slot 0 in front of it (head), an odd end
// leaves slot L - 1 behind it (tail).  The body goes out in chunks of kChunkUnits = kUnroll x kWave
// units, `c[u]` of lane l being row u of the chunk:
//   * chunk ci, row u, lane l holds unit ci * kChunkUnits + u * kWave + l of the body: .x is slot
//     s0 + 2 * that (s0 = a0 - beg, 0 or 1) and .y the slot after it.  Slots therefore ascend in
//     (chunk, row, lane, .x before .y) order;
//   * nfull full chunks come first.  One partial chunk follows when units remain (rem of them) or
//     there is a head or a tail.  Its units past the body are NaN, a full chunk has none;
//   * lane kWave - 1 of row kUnroll - 1 of the partial chunk (a unit the body never reaches there)
//     holds slot 0 in .x when there is a head and slot L - 1 in .y when there is a tail, each NaN
//     otherwise;
//   * a NaN is absent to every processor; padding() counts the ones that are no slot at all.
#pragma once

#include <stdint.h>

#include "krr_plan.h"  // kUnroll, kWave, KRR_HD

namespace krr {

// always inlined: the layout is part of the loop it describes
#define KRR_GEOM KRR_HD inline __attribute__((always_inline))

constexpr int kChunkUnits = kUnroll * kWave;  // double2 units per chunk

struct SegGeom {
    int64_t a0, a1;   // the body is values[a0, a1)
    int64_t s0;       // slot of the body's first unit: a0 - beg
    int64_t i0;       // ... and its index among the double2 units of values: a0 / 2
    int64_t nunits;   // units of the body
    int64_t nfull;    // full chunks
    int32_t rem;      // body units of the partial chunk
    bool head, tail;  // slot 0 / slot L - 1 lies outside the body
    bool part;        // there is a partial chunk: rem > 0 || head || tail
    KRR_GEOM bool partial() const { return part; }
    KRR_GEOM int64_t nch() const { return nfull + (partial() ? 1 : 0); }
    KRR_GEOM uint32_t padding() const {  // NaNs of the partial chunk that are no slot
        return partial() ? (uint32_t)(2 * kChunkUnits - 2 * rem - (head ? 1 : 0) - (tail ? 1 : 0)) : 0u;
    }
    // The contract's position rules, for the CPU test of its arithmetic; the kernels use the fields
    // above and a SegCursor, and what the loops load where stays with the GPU tests.
    // slot in .x of chunk ci, row u, lane l, unless that is the edge unit
    KRR_GEOM int64_t slot(int64_t ci, int u, int l) const { return s0 + 2 * (ci * kChunkUnits + u * kWave + l); }
    // the unit that holds (slot 0, slot L - 1) instead
    KRR_GEOM bool edge(int64_t ci, int u, int l) const {
        return partial() && ci == nfull && u == kUnroll - 1 && l == kWave - 1;
    }
};

KRR_GEOM SegGeom seg_geom(int64_t beg, int64_t end) {
    int64_t a0 = (beg + 1) & ~(int64_t)1;
    if (a0 > end) a0 = end;
    int64_t a1 = end & ~(int64_t)1;
    if (a1 < a0) a1 = a0;
    const int64_t i0 = a0 >> 1;
    const int64_t nunits = (a1 >> 1) - i0;
    const int64_t nfull = nunits / kChunkUnits;
    const int64_t rem = nunits - nfull * kChunkUnits;
    const bool head = a0 > beg, tail = a1 < end;
    const bool part = rem > 0 || head || tail;
    return SegGeom{a0, a1, a0 - beg, i0, nunits, nfull, (int32_t)rem, head, tail, part};
}

// proc.chunk(c) carries no position: a processor that needs one counts its chunks with this.
struct SegCursor {
    uint32_t full;  // full chunks still to come before the partial one (2^32 chunks are 32 TiB: never reached)
    int64_t base;  // slot of lane 0's c[0].x in the chunk to come
    int lane;
    KRR_GEOM SegCursor(const SegGeom& g, int lane_) : full((uint32_t)g.nfull), base(g.s0), lane(lane_) {}
    KRR_GEOM bool partial() const { return full == 0; }  // the chunk in hand is the partial one (wave-uniform)
    KRR_GEOM bool edge_row(int u) const { return partial() && u == kUnroll - 1; }  // its row with the edge unit
    KRR_GEOM bool edge(int u) const { return edge_row(u) && lane == kWave - 1; }   // this lane's c[u] is that unit
    KRR_GEOM int64_t row_base(int u) const { return base + 2 * kWave * u; }        // slot of lane 0's c[u].x
    KRR_GEOM void next() {  // after every chunk
        base += 2 * kChunkUnits;
        --full;
    }
};

}  // namespace krr
