// plan_layout.hpp -- the host combinatorics of plan creation (csrc/gridder.hip: create_impl): how the tile-sorted
// visibilities are cut into work items and colour slices, and which rows, tiles, column runs and row spans of the uv-plane
// the items' footprints reach.  Plain C++17 on values and vectors: no HIP, no handle, so every function here is tested on
// the CPU (tests/test_plan_layout_cpu.py) against a per-cell / per-visibility restatement.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

namespace pfbhip {

constexpr int TILE = 32;     // uv tile edge in grid cells
constexpr int TP = 32;       // transpose tile
constexpr int CHUNK = 4096;  // sorted visibilities per work item
static_assert(TP == TILE, "row-block occupancy assumes transpose tile == uv tile");

struct WorkItem {
    uint32_t tile, begin, end, pad;
};

// (row0, nrows, col0, ncols) of a clear rectangle, (begin, end, begin, end) of a tile row's two column runs: uploaded as int4
struct alignas(16) Int4 {
    int x, y, z, w;
};

// a footprint region that does not map to consecutive tiles (the caller reports it as an invalid argument)
struct LayoutError : std::logic_error {
    using std::logic_error::logic_error;
};

// visibilities per work item (<= CHUNK): smaller items balance the launch tail, larger ones amortise the per-item
// prologue / tile flush
inline uint32_t gather_chunk(int wmode, int64_t nactive)
{
    uint32_t chunk = CHUNK;
    if (wmode == 2) {  // the one-plane gather (256-thread workgroups, 768 slots): about three items per slot, 512..4096 each
        chunk = 512;
        while (chunk < CHUNK && double(chunk) * 1.5 < double(nactive) / (3.0 * 768.0)) chunk *= 2;
    }
    return chunk;
}

// The one-plane scatter runs 256-thread workgroups: an item of 4096 visibilities is 1024 per wave, longer than a whole
// colour launch of a mid-size plan should take (4096^2, 4e6 visibilities: grid 1.61 ms -> 1.02 with items of <= 1024; C2
// indifferent between 1024 and 4096).  Its lists are cut finer than the gather's: about three items per workgroup
// slot and launch, 512..2048 visibilities each.
inline uint32_t scatter_chunk(int wmode, int64_t nactive, bool coloured, uint32_t gather_chunk)
{
    uint32_t schunk = gather_chunk;
    if (wmode == 2) {
        const double per_launch = double(nactive) / (coloured ? 4.0 : 1.0);
        uint32_t c = 512;
        while (c < 2048 && double(c) * 1.5 < per_launch / (3.0 * 768.0)) c *= 2;
        schunk = std::min(c, gather_chunk);
    }
    return schunk;
}

struct WorkLists {
    std::vector<WorkItem> work;
    std::vector<size_t> work_off, work_cnt;  // per pass of kp_max planes (one pass unless plane-sorted)
    size_t coarse_items = 0;  // work items at CHUNK visibilities each (the size measure of the launch-shape decisions)
};

// The work items of every pass from the starts of the sort keys (tstart: ntiles * key_planes + 1 entries; empty: a plan
// without visibilities, one pass without items).
inline WorkLists split_work(const std::vector<uint32_t> &tstart, int64_t ntiles, int64_t key_planes, int64_t nplanes, int W, int kp_max,
                            bool plane_sorted, uint32_t chunk)
{
    WorkLists out;
    auto &work = out.work;
    const int64_t P = key_planes, ngroups = (nplanes + kp_max - 1) / kp_max;
    for (int64_t grp = 0; grp < (plane_sorted ? ngroups : 1) && !tstart.empty(); ++grp) {
        // planes [q, q + kp) are touched by visibilities whose first plane lies in [q - W + 1, q + kp - 1]
        const int64_t q = grp * kp_max, kp = std::min<int64_t>(kp_max, nplanes - q);
        const int64_t lo_p = plane_sorted ? std::max<int64_t>(0, q - W + 1) : 0;
        const int64_t hi_p = plane_sorted ? std::min<int64_t>(P - 1, q + kp - 1) : 0;
        const size_t first = work.size();
        for (int64_t t = 0; t < ntiles; ++t) {
            const uint32_t b0 = tstart[size_t(t * P + lo_p)], b1 = tstart[size_t(t * P + hi_p + 1)];
            // a tile's visibilities in equal parts of <= chunk (4096 + 904 would leave a short item behind a long one)
            const uint32_t nt = b1 - b0, parts = (nt + chunk - 1) / chunk;
            out.coarse_items += (nt + CHUNK - 1) / CHUNK;
            for (uint32_t i = 0; i < parts; ++i)
                work.push_back(WorkItem{uint32_t(t), b0 + uint32_t(uint64_t(nt) * i / parts), b0 + uint32_t(uint64_t(nt) * (i + 1) / parts), 0});
        }
        // Longest-processing-time-first: heavy chunks are dispatched first, the many tiny ones of the
        // sparse outer uv-plane fill the tail (the uv density is strongly peaked at the centre).
        std::stable_sort(work.begin() + std::ptrdiff_t(first), work.end(),
                         [](const WorkItem &x, const WorkItem &y) { return (x.end - x.begin) > (y.end - y.begin); });
        out.work_off.push_back(first);
        out.work_cnt.push_back(work.size() - first);
    }
    if (out.work_off.empty()) {
        out.work_off.push_back(0);
        out.work_cnt.push_back(0);
    }
    return out;
}

struct ColourSlices {
    std::vector<WorkItem> wcol;
    std::vector<size_t> col_off, col_cnt;  // four slices per pass
};

// colour slices of every group's list (LPT order kept inside a slice); chunks of a tile that has several in the
// slice are flagged shared (pad = 1) and keep the atomic flush
inline ColourSlices colour_slices(const std::vector<WorkItem> &work, const std::vector<size_t> &work_off, const std::vector<size_t> &work_cnt,
                                  int64_t ntiles, int ntv, bool coloured, uint32_t schunk, uint32_t chunk)
{
    ColourSlices out;
    auto &wcol = out.wcol;
    wcol.reserve(work.size());
    std::vector<uint32_t> seen;
    for (size_t grp = 0; grp < work_off.size(); ++grp) {
        const size_t b0 = work_off[grp], b1 = b0 + work_cnt[grp];
        seen.assign(size_t(ntiles), 0);
        for (size_t i = b0; i < b1; ++i) seen[work[i].tile]++;
        for (int col = 0; col < 4; ++col) {
            out.col_off.push_back(wcol.size());
            for (size_t i = b0; i < b1; ++i) {
                const uint32_t tu = work[i].tile / uint32_t(ntv), tv = work[i].tile % uint32_t(ntv);
                const int c = coloured ? int((tu & 1u) * 2u + (tv & 1u)) : 0;
                if (c != col) continue;
                WorkItem w = work[i];
                const uint32_t nt = w.end - w.begin, parts = (nt + schunk - 1) / schunk;
                w.pad = (!coloured || seen[w.tile] > 1 || parts > 1) ? 1u : 0u;
                for (uint32_t q = 0; q < std::max(parts, 1u); ++q) {
                    WorkItem wq = w;
                    wq.begin = w.begin + uint32_t(uint64_t(nt) * q / std::max(parts, 1u));
                    wq.end = w.begin + uint32_t(uint64_t(nt) * (q + 1) / std::max(parts, 1u));
                    wcol.push_back(wq);
                }
            }
            if (schunk < chunk)  // (the finer split interleaves the parts of neighbouring items: heaviest first again)
                std::stable_sort(wcol.begin() + std::ptrdiff_t(out.col_off.back()), wcol.end(),
                                 [](const WorkItem &x, const WorkItem &y) { return (x.end - x.begin) > (y.end - y.begin); });
            out.col_cnt.push_back(wcol.size() - out.col_off.back());
        }
    }
    if (out.col_off.empty()) {
        out.col_off.assign(4, 0);
        out.col_cnt.assign(4, 0);
    }
    return out;
}

// occupancy of 32-row blocks of the uv-plane: tile rows that hold work, plus the block their
// (W-1)-cell halo spills into
// (every block a footprint row can fall in: with a short last block -- nu % 32 < W - 1 -- the footprints of the tile
// before it run THROUGH that block and wrap into block 0; marking only the first and the last row's block left it out)
inline std::vector<uint8_t> row_block_occupancy(const std::vector<WorkItem> &work, int ntv, int64_t nu, int W)
{
    const int64_t nblk = (nu + TP - 1) / TP;
    std::vector<uint8_t> occ(size_t(nblk), 0);
    for (const WorkItem &wi : work) {
        const int64_t tu = wi.tile / uint32_t(ntv);
        for (int64_t r = tu * TILE; r <= tu * TILE + TILE + W - 2; ++r) occ[size_t((r % nu) / TP)] = 1;
    }
    return occ;
}

// tiles a footprint cell of some work item can fall in (the item's own tile and the tiles its (W - 1)-cell halo reaches,
// wrapped; through a short last tile if the grid size is not a multiple of TILE).  Per TILE with work, and per row /
// column of its region rather than per cell: the per-cell, per-item form of this loop was 0.1 s of the 0.13 s a C2 plan
// takes and 3.1 s of C5's 3.3 (18 449 / 400 000 work items x 47^2 cells x two passes).  Empty without work.
inline std::vector<uint8_t> touched_tiles(const std::vector<WorkItem> &work, int64_t ntiles, int ntv, int64_t nu, int64_t nv, int W)
{
    std::vector<uint8_t> touched;
    if (work.empty()) return touched;
    const int64_t ntu = (nu + TILE - 1) / TILE;
    touched.assign(size_t(ntu * ntv), 0);
    std::vector<uint8_t> seen(size_t(ntiles), 0);
    for (const WorkItem &wi : work) {
        if (seen[wi.tile]) continue;
        seen[wi.tile] = 1;
        const int64_t tu = wi.tile / uint32_t(ntv), tv = wi.tile % uint32_t(ntv);
        constexpr int MAXT = 8;  // (own tile, short last tile, tile 0, ...: four on the smallest grids)
        int64_t tr[MAXT], tc[MAXT];
        int ntr = 0, ntc = 0;
        for (int64_t r = tu * TILE; r <= tu * TILE + TILE + W - 2; ++r) {
            const int64_t t = (r % nu) / TILE;
            if (ntr == 0 || (tr[ntr - 1] != t && ntr < MAXT)) tr[ntr++] = t;
            if (tr[ntr - 1] != t) throw LayoutError("tile rows of a footprint region");
        }
        for (int64_t q = tv * TILE; q <= tv * TILE + TILE + W - 2; ++q) {
            const int64_t t = (q % nv) / TILE;
            if (ntc == 0 || (tc[ntc - 1] != t && ntc < MAXT)) tc[ntc++] = t;
            if (tc[ntc - 1] != t) throw LayoutError("tile columns of a footprint region");
        }
        for (int a = 0; a < ntr; ++a)
            for (int b = 0; b < ntc; ++b) touched[size_t(tr[a] * ntv + tc[b])] = 1;
    }
    return touched;
}

struct ColumnRuns {
    std::vector<Int4> runs_t;  // per tile row: its first two runs (begin, end, begin, end)
    std::vector<Int4> rects;   // the runs' cells in rectangles of <= 8 rows: (row0, nrows, col0, ncols)
    int64_t cells = 0, full = 0;  // area of the rectangles; whole rows of the tile rows that have any
};

// Column runs per tile row: the runs of touched tile columns, the whole row for three or more runs (or without work:
// `touched` empty).
inline ColumnRuns column_runs(const std::vector<uint8_t> &touched, int64_t nu, int64_t nv, int ntv)
{
    const int64_t ntu = (nu + TILE - 1) / TILE;
    ColumnRuns out;
    out.runs_t.assign(size_t(ntu), Int4{0, int(nv), 0, 0});
    if (touched.empty()) return out;
    constexpr int SLICE = 8;  // rows per rectangle: enough workgroups to fill the chip
    for (int64_t tu = 0; tu < ntu; ++tu) {
        std::vector<std::pair<int, int>> rr;
        for (int64_t tv = 0; tv < ntv;) {
            if (!touched[size_t(tu * ntv + tv)]) { ++tv; continue; }
            int64_t e = tv;
            while (e < ntv && touched[size_t(tu * ntv + e)]) ++e;
            rr.emplace_back(int(tv * TILE), int(std::min<int64_t>(e * TILE, nv)));
            tv = e;
        }
        if (rr.size() >= 3) rr.assign(1, {0, int(nv)});
        const int row0 = int(tu * TILE), nrows = int(std::min<int64_t>(TILE, nu - row0));
        for (auto &run : rr) {
            const int col0 = run.first, ncols = run.second - run.first;
            for (int q = 0; q < nrows; q += SLICE) out.rects.push_back(Int4{row0 + q, std::min(SLICE, nrows - q), col0, ncols});
            out.cells += int64_t(nrows) * ncols;
        }
        if (!rr.empty()) out.full += int64_t(nrows) * nv;
        rr.resize(2, {0, 0});
        out.runs_t[size_t(tu)] = Int4{rr[0].first, rr[0].second, rr[1].first, rr[1].second};
    }
    return out;
}

// spans of consecutive occupied blocks (at most a handful for a centrally concentrated uv coverage) as (row0, nrows), the
// last one clipped to nu; more than four: fragmented coverage, everything counts as occupied (occ is set accordingly)
inline std::vector<std::pair<int64_t, int64_t>> occupied_spans(std::vector<uint8_t> &occ, int64_t nu)
{
    const int64_t nblk = int64_t(occ.size());
    std::vector<std::pair<int64_t, int64_t>> runs;
    for (int64_t bk = 0; bk < nblk;) {
        if (!occ[size_t(bk)]) { ++bk; continue; }
        int64_t e = bk;
        while (e < nblk && occ[size_t(e)]) ++e;
        runs.emplace_back(bk, e);
        bk = e;
    }
    if (runs.size() > 4) {  // fragmented coverage: transform everything
        std::fill(occ.begin(), occ.end(), uint8_t(1));
        runs.assign(1, {0, nblk});
    }
    for (auto &r : runs) {
        const int64_t row0 = r.first * TP;
        r = {row0, std::min<int64_t>(r.second * TP, nu) - row0};
    }
    return runs;
}

// block id -> row of the transposing first-axis transforms over the occupied rows (spans: (row0, nrows)): consecutive
// block ids go to the 8 XCDs in turn, so a super-group of 64 ids gives every XCD 8 adjacent rows; the tail keeps its order
inline std::vector<int> xcd_row_map(const std::vector<std::pair<int64_t, int64_t>> &spans)
{
    std::vector<int> rows;
    for (auto &sp : spans)
        for (int64_t r = 0; r < sp.second; ++r) rows.push_back(int(sp.first + r));
    const size_t n = rows.size(), ngroups = n / 8, nfull = ngroups / 8;
    std::vector<int> map(n);
    for (size_t b = 0; b < n; ++b) {
        if (b < nfull * 64) {  // super-group of 64 block ids = 8 XCDs x 8 adjacent rows
            const size_t sg = b / 64, r = b % 64, xcd = r % 8, k = r / 8;
            map[b] = rows[(sg * 8 + xcd) * 8 + k];
        } else {
            map[b] = rows[b];
        }
    }
    return map;
}

// one-plane scheme: the kernel polynomial table (W pieces of D1 monomial coefficients) and its K - 1 even derivatives
inline std::vector<double> wd_derivative_table(const std::vector<double> &ktab, int K, int W, int D1)
{
    std::vector<double> dtab(size_t(K) * W * D1, 0.0);
    std::copy(ktab.begin(), ktab.end(), dtab.begin());
    // x = (a + 1 - W/2 - (z + 1) / 2) 2 / W  =>  d^2/dx^2 = W^2 d^2/dz^2
    for (int k = 1; k < K; ++k)
        for (int a = 0; a < W; ++a) {
            const double *src = &dtab[(size_t(k - 1) * W + a) * D1];
            double *dst = &dtab[(size_t(k) * W + a) * D1];
            for (int q = 0; q + 2 < D1; ++q) dst[q] = src[q + 2] * double((q + 2) * (q + 1)) * double(W) * double(W);
        }
    return dtab;
}

}  // namespace pfbhip
