// Host build of the streaming layout (krr_amd/csrc/krr_geom.h) for the CPU tests
// (tests/test_segment_geom.py): seg_geom's numbers, and what every (chunk, row, lane, half) of a
// segment holds, composed from the header's own position functions.  Test infrastructure only.
#include <stdint.h>

#include "krr_geom.h"

using namespace krr;

// out[12]: a0, a1, s0, i0, nunits, nfull, rem, head, tail, partial(), nch(), padding()
extern "C" void geom_check_geom(int64_t beg, int64_t end, int64_t* out) {
    const SegGeom g = seg_geom(beg, end);
    const int64_t v[12] = {g.a0,  g.a1,  g.s0,  g.i0,  g.nunits,    g.nfull,
                           g.rem, g.head, g.tail, g.partial(), g.nch(), (int64_t)g.padding()};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
}

// out[nch() * kUnroll * kWave * 2], in (chunk, row, lane, .x / .y) order: the slot held, -1 for a
// NaN that is no slot.  A unit past the body is padding; the edge unit holds (slot 0, slot L - 1)
// where there is a head / a tail.  Returns nch(), or -1 when cap is too small.
extern "C" int64_t geom_check_layout(int64_t beg, int64_t end, int64_t* out, int64_t cap) {
    const SegGeom g = seg_geom(beg, end);
    if (g.nch() * 2 * kChunkUnits > cap) return -1;
    int64_t k = 0;
    for (int64_t ci = 0; ci < g.nch(); ++ci)
        for (int u = 0; u < kUnroll; ++u)
            for (int l = 0; l < kWave; ++l, k += 2) {
                const bool body = ci * kChunkUnits + u * kWave + l < g.nunits;
                out[k] = body ? g.slot(ci, u, l) : -1;
                out[k + 1] = body ? g.slot(ci, u, l) + 1 : -1;
                if (g.edge(ci, u, l)) {
                    out[k] = g.head ? 0 : -1;
                    out[k + 1] = g.tail ? end - beg - 1 : -1;
                }
            }
    return g.nch();
}

// A SegCursor of lane `lane` walked over the segment's chunks: per chunk its row_base(u) [kUnroll],
// and bit u of edge_rows / edges set where edge_row(u) / edge(u) is.
extern "C" void geom_check_cursor(int64_t beg, int64_t end, int lane, int64_t* row_base, int32_t* edge_rows,
                                  int32_t* edges) {
    const SegGeom g = seg_geom(beg, end);
    SegCursor at(g, lane);
    for (int64_t ci = 0; ci < g.nch(); ++ci, at.next()) {
        edge_rows[ci] = edges[ci] = 0;
        for (int u = 0; u < kUnroll; ++u) {
            row_base[ci * kUnroll + u] = at.row_base(u);
            edge_rows[ci] |= (at.edge_row(u) ? 1 : 0) << u;
            edges[ci] |= (at.edge(u) ? 1 : 0) << u;
        }
    }
}
