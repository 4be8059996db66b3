"""CPU tests of csrc/plan_layout.hpp, the host combinatorics of plan creation: work items, colour slices, row-block
occupancy, touched tiles, column runs, row spans, the XCD row map, the chunk rules and the derivative table.

A small stand-alone program (its own main, host g++, no HIP) reads one command per line and prints what the header's
function returns; every result is checked here against a naive restatement per cell / per visibility index written in
Python.  The program is built once, and once more with the address and undefined-behaviour sanitizers linked statically
(index arithmetic); both builds must print the same."""

import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pfb-imaging_amd", "csrc")
TILE, TP, CHUNK = 32, 32, 4096

DRIVER = r"""
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "plan_layout.hpp"
using namespace pfbhip;

static std::vector<WorkItem> read_items(std::istream &in)
{
    size_t n;
    in >> n;
    std::vector<WorkItem> w(n);
    for (auto &x : w) in >> x.tile >> x.begin >> x.end;
    return w;
}
static void print_items(const std::vector<WorkItem> &w)
{
    printf(" %zu", w.size());
    for (auto &x : w) printf(" %u %u %u %u", x.tile, x.begin, x.end, x.pad);
}
template <class T>
static std::vector<T> read_vec(std::istream &in)
{
    size_t n;
    in >> n;
    std::vector<T> v(n);
    for (auto &x : v) {
        double d;
        in >> d;
        x = T(d);
    }
    return v;
}

int main()
{
    static_assert(TILE == 32 && TP == 32 && CHUNK == 4096 && sizeof(WorkItem) == 16 && sizeof(Int4) == 16, "constants");
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "split_work") {
            long long ntiles, P, nplanes;
            int W, kp_max, sorted;
            unsigned chunk;
            in >> ntiles >> P >> nplanes >> W >> kp_max >> sorted >> chunk;
            auto tstart = read_vec<uint32_t>(in);
            WorkLists o = split_work(tstart, ntiles, P, nplanes, W, kp_max, sorted != 0, chunk);
            printf("%zu %zu", o.coarse_items, o.work_off.size());
            for (size_t g = 0; g < o.work_off.size(); ++g) printf(" %zu %zu", o.work_off[g], o.work_cnt[g]);
            print_items(o.work);
        } else if (cmd == "colour_slices") {
            long long ntiles;
            int ntv, coloured;
            unsigned schunk, chunk;
            in >> ntiles >> ntv >> coloured >> schunk >> chunk;
            auto off = read_vec<size_t>(in), cnt = read_vec<size_t>(in);
            auto work = read_items(in);
            ColourSlices o = colour_slices(work, off, cnt, ntiles, ntv, coloured != 0, schunk, chunk);
            printf("%zu", o.col_off.size());
            for (size_t g = 0; g < o.col_off.size(); ++g) printf(" %zu %zu", o.col_off[g], o.col_cnt[g]);
            print_items(o.wcol);
        } else if (cmd == "row_block_occupancy") {
            int ntv, W;
            long long nu;
            in >> ntv >> nu >> W;
            for (auto b : row_block_occupancy(read_items(in), ntv, nu, W)) printf("%d ", int(b));
        } else if (cmd == "touched_tiles") {
            long long ntiles, nu, nv;
            int ntv, W;
            in >> ntiles >> ntv >> nu >> nv >> W;
            try {
                for (auto b : touched_tiles(read_items(in), ntiles, ntv, nu, nv, W)) printf("%d ", int(b));
            } catch (const LayoutError &e) {
                printf("error %s", e.what());
            }
        } else if (cmd == "column_runs") {
            long long nu, nv;
            int ntv;
            in >> nu >> nv >> ntv;
            ColumnRuns o = column_runs(read_vec<uint8_t>(in), nu, nv, ntv);
            printf("%lld %lld %zu", (long long)o.cells, (long long)o.full, o.runs_t.size());
            for (auto &r : o.runs_t) printf(" %d %d %d %d", r.x, r.y, r.z, r.w);
            printf(" %zu", o.rects.size());
            for (auto &r : o.rects) printf(" %d %d %d %d", r.x, r.y, r.z, r.w);
        } else if (cmd == "occupied_spans") {
            long long nu;
            in >> nu;
            auto occ = read_vec<uint8_t>(in);
            auto sp = occupied_spans(occ, nu);
            printf("%zu", sp.size());
            for (auto &s : sp) printf(" %lld %lld", (long long)s.first, (long long)s.second);
            for (auto b : occ) printf(" %d", int(b));
        } else if (cmd == "xcd_row_map") {
            size_t n;
            in >> n;
            std::vector<std::pair<int64_t, int64_t>> sp(n);
            for (auto &s : sp) in >> s.first >> s.second;
            for (int r : xcd_row_map(sp)) printf("%d ", r);
        } else if (cmd == "chunks") {
            int wmode, coloured;
            long long nactive;
            in >> wmode >> nactive >> coloured;
            const uint32_t gc = gather_chunk(wmode, nactive);
            printf("%u %u", gc, scatter_chunk(wmode, nactive, coloured != 0, gc));
        } else if (cmd == "wd_derivative_table") {
            int K, W, D1;
            in >> K >> W >> D1;
            for (double d : wd_derivative_table(read_vec<double>(in), K, W, D1)) printf("%.17g ", d);
        } else {
            printf("unknown command");
            return 2;
        }
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """(plain program, sanitized program or None where the toolchain cannot link the sanitizers' static runtimes)"""
    d = tmp_path_factory.mktemp("plan_layout")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    base = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src)]
    subprocess.check_call(base + ["-o", str(d / "driver")])
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                                 "-o", str(d / "driver_san")], capture_output=True)
    return str(d / "driver"), (str(d / "driver_san") if san.returncode == 0 else None)


class Driver:
    def __init__(self, builds):
        self.exe, self.san = builds
        self.lines = []

    def ask(self, *words):
        self.lines.append(" ".join(str(w) for w in words))
        return len(self.lines) - 1

    def run(self):
        text = "\n".join(self.lines) + "\n"
        out = subprocess.run([self.exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        if self.san is not None:
            env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
            chk = subprocess.run([self.san], input=text, capture_output=True, text=True, env=env)
            assert chk.returncode == 0, chk.stderr[-2000:]
            assert chk.stdout.split("\n") == out
        return out[:len(self.lines)]


@pytest.fixture()
def drv(builds):
    return Driver(builds)


def vec(v):
    v = list(v)
    return [len(v)] + [int(x) for x in v]


def items_arg(items):
    return [len(items)] + [x for it in items for x in it[:3]]


def parse_items(tok, pos):
    n = int(tok[pos])
    flat = [int(x) for x in tok[pos + 1:pos + 1 + 4 * n]]
    return [tuple(flat[4 * i:4 * i + 4]) for i in range(n)], pos + 1 + 4 * n


def parse_split(line):
    tok = line.split()
    coarse, ng = int(tok[0]), int(tok[1])
    groups = [(int(tok[2 + 2 * g]), int(tok[3 + 2 * g])) for g in range(ng)]
    work, end = parse_items(tok, 2 + 2 * ng)
    assert end == len(tok)
    return coarse, groups, work


def ceil_div(a, b):
    return -(-a // b)


# ---- split_work -------------------------------------------------------------------------------------------------------------
TILE_COUNTS = (0, 1, 512, 513, 4096 + 904, 3, 4096, 4097, 0, 2 * 4096 + 1)


def _tstart(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@pytest.mark.parametrize("chunk", [512, 4096])
def test_split_work_one_pass(drv, chunk):
    counts = [c if c not in (512, 513) else c - 512 + chunk for c in TILE_COUNTS]  # 0, 1, chunk, chunk + 1, 4096 + 904, ...
    ts = _tstart(counts)
    drv.ask("split_work", len(counts), 1, 7, 8, 4, 0, chunk, *vec(ts))
    coarse, groups, work = parse_split(drv.run()[0])
    assert groups == [(0, len(work))]
    _check_group(work, ts, len(counts), 1, 0, 0, chunk)
    assert coarse == sum(ceil_div(c, CHUNK) for c in counts)
    assert all(it[3] == 0 for it in work)


def _check_group(items, ts, ntiles, P, lo_p, hi_p, chunk):
    """the items of one pass: per tile an exact partition of [ts[t P + lo_p], ts[t P + hi_p + 1]) into parts of <= chunk whose
    sizes differ by at most one; the pass in non-increasing size order, the (tile, begin) order kept among equal sizes"""
    per_tile = {}
    for tile, b, e, _ in items:
        per_tile.setdefault(tile, []).append((b, e))
    for t in range(ntiles):
        b0, b1 = int(ts[t * P + lo_p]), int(ts[t * P + hi_p + 1])
        parts = sorted(per_tile.get(t, []))
        covered = [i for b, e in parts for i in range(b, e)]
        assert covered == list(range(b0, b1)), t  # every visibility index once, nothing outside
        sizes = [e - b for b, e in parts]
        assert all(0 < s <= chunk for s in sizes), (t, sizes)
        assert not sizes or max(sizes) - min(sizes) <= 1, (t, sizes)
        assert len(parts) == ceil_div(b1 - b0, chunk)  # (no more parts than the size bound needs)
    sizes = [e - b for _, b, e, _ in items]
    assert sizes == sorted(sizes, reverse=True)
    for s, grp in itertools.groupby(items, key=lambda it: it[2] - it[1]):
        keys = [(it[0], it[1]) for it in grp]
        assert keys == sorted(keys), s  # stable: the order of generation (tile, then begin) among equal sizes


def test_split_work_plane_sorted(drv):
    """11 planes, W = 4, 4 planes per pass: passes of planes [0, 4), [4, 8), [8, 11) read first planes [0, 3], [1, 7], [5, 10]
    (clipped at 0 and at P - 1)"""
    rng = np.random.default_rng(3)
    P, W, kp, chunk, ntiles = 11, 4, 4, 512, len(TILE_COUNTS)
    counts = []
    for c in TILE_COUNTS:  # a tile's visibilities over its 11 first planes
        counts += list(rng.multinomial(c, np.full(P, 1.0 / P)))
    ts = _tstart(counts)
    drv.ask("split_work", ntiles, P, P, W, kp, 1, chunk, *vec(ts))
    coarse, groups, work = parse_split(drv.run()[0])
    ranges = [(0, 3), (1, 7), (5, 10)]
    assert len(groups) == 3 and groups[0][0] == 0
    want_coarse = 0
    for (off, cnt), (lo, hi) in zip(groups, ranges):
        _check_group(work[off:off + cnt], ts, ntiles, P, lo, hi, chunk)
        want_coarse += sum(ceil_div(int(ts[t * P + hi + 1] - ts[t * P + lo]), CHUNK) for t in range(ntiles))
    assert [g[0] for g in groups] == list(np.cumsum([0] + [g[1] for g in groups[:-1]]))
    assert sum(g[1] for g in groups) == len(work) and coarse == want_coarse


def test_split_work_without_visibilities(drv):
    drv.ask("split_work", 12, 1, 3, 8, 3, 0, 4096, 0)
    assert parse_split(drv.run()[0]) == (0, [(0, 0)], [])


# ---- colour_slices ----------------------------------------------------------------------------------------------------------
def _random_work(rng, ntiles, chunk, groups=2):
    """work lists as split_work makes them (several items on some tiles, none on others), per pass"""
    work, off, cnt = [], [], []
    pos = 0
    for _ in range(groups):
        first = len(work)
        for t in range(ntiles):
            n = int(rng.choice([0, 1, chunk, chunk + 1, 3 * chunk - 5, 700]))
            parts = ceil_div(n, chunk)
            for q in range(parts):
                work.append((t, pos + n * q // parts, pos + n * (q + 1) // parts))
            pos += n
        work[first:] = sorted(work[first:], key=lambda it: -(it[2] - it[1]))
        off.append(first)
        cnt.append(len(work) - first)
    return work, off, cnt


@pytest.mark.parametrize("ntu,ntv,coloured", [(2, 2, True), (4, 2, True), (3, 3, False), (2, 2, False)])
@pytest.mark.parametrize("chunk,schunk", [(4096, 4096), (4096, 1024), (512, 512)])
def test_colour_slices(drv, ntu, ntv, coloured, chunk, schunk):
    rng = np.random.default_rng(ntu * 10 + ntv)
    work, off, cnt = _random_work(rng, ntu * ntv, chunk)
    drv.ask("colour_slices", ntu * ntv, ntv, int(coloured), schunk, chunk, *vec(off), *vec(cnt), *items_arg(work))
    tok = drv.run()[0].split()
    nsl = int(tok[0])
    assert nsl == 4 * len(off)
    slices = [(int(tok[1 + 2 * s]), int(tok[2 + 2 * s])) for s in range(nsl)]
    wcol, end = parse_items(tok, 1 + 2 * nsl)
    assert end == len(tok)
    assert [s[0] for s in slices] == list(np.cumsum([0] + [s[1] for s in slices[:-1]])) and sum(s[1] for s in slices) == len(wcol)
    for g in range(len(off)):
        group = work[off[g]:off[g] + cnt[g]]
        per_tile = {}
        for t, b, e in group:
            per_tile[t] = per_tile.get(t, 0) + 1
        seen = []
        for col in range(4):
            o, n = slices[4 * g + col]
            sl = wcol[o:o + n]
            for t, b, e, pad in sl:
                assert col == (((t // ntv) & 1) * 2 + ((t % ntv) & 1) if coloured else 0)
                assert 0 < e - b <= schunk
                # the parent item: the one of this pass that holds [b, e)
                (parent,) = [it for it in group if it[0] == t and it[1] <= b and e <= it[2]]
                split_further = (parent[1], parent[2]) != (b, e)
                assert pad == (0 if (coloured and per_tile[t] == 1 and not split_further) else 1)
                seen += range(b, e)
            if schunk < chunk:
                sizes = [e - b for _, b, e, _ in sl]
                assert sizes == sorted(sizes, reverse=True)
            else:  # nothing is cut: the pass's order is kept inside a slice
                assert [it[:3] for it in sl] == [it for it in group if (((it[0] // ntv) & 1) * 2 + ((it[0] % ntv) & 1) if coloured else 0) == col]
        assert sorted(seen) == sorted(i for _, b, e in group for i in range(b, e))  # every index of the pass exactly once


def test_colour_slices_parts_are_even(drv):
    """an item cut for the scatter: parts of <= schunk whose sizes differ by at most one"""
    work = [(0, 10, 10 + 4096), (3, 5000, 5000 + 2049), (1, 8000, 8001)]
    drv.ask("colour_slices", 4, 2, 1, 1024, 4096, *vec([0]), *vec([3]), *items_arg(work))
    tok = drv.run()[0].split()
    wcol, _ = parse_items(tok, 9)
    for t, b0, b1 in work:
        parts = sorted((b, e) for tt, b, e, _ in wcol if tt == t)
        assert [i for b, e in parts for i in range(b, e)] == list(range(b0, b1))
        sizes = [e - b for b, e in parts]
        assert len(sizes) == ceil_div(b1 - b0, 1024) and max(sizes) - min(sizes) <= 1


def test_colour_slices_without_work(drv):
    drv.ask("colour_slices", 4, 2, 1, 512, 512, *vec([0]), *vec([0]), 0)
    assert drv.run()[0].split() == ["4"] + ["0"] * 8 + ["0"]


# ---- row_block_occupancy, touched_tiles -------------------------------------------------------------------------------------
GRIDS = [((40, 64), None), ((32, 32), None), ((72, 96), None), ((8, 8), None), ((128, 128), [(3, 0)])]


def _footprint_cells(tu, tv, nu, nv, W):
    """every cell a visibility of tile (tu, tv) can touch: origin anywhere in the tile, W taps per axis, wrapped"""
    return {((tu * TILE + a) % nu, (tv * TILE + b) % nv) for a in range(TILE + W - 1) for b in range(TILE + W - 1)}


@pytest.mark.parametrize("W", [16, 4])
@pytest.mark.parametrize("grid,only", GRIDS)
def test_occupancy_and_touched_tiles_per_cell(drv, grid, only, W):
    nu, nv = grid
    ntu, ntv = ceil_div(nu, TILE), ceil_div(nv, TILE)
    tiles = [(tu, tv) for tu in range(ntu) for tv in range(ntv)]
    # every single tile alone, the given selection, every tile at once (two items on the first: seen once)
    selections = [[t] for t in tiles] if only is None else []
    selections += [only or tiles, (only or tiles) + (only or tiles)[:1]]
    for sel in selections:
        items = [(tu * ntv + tv, 0, 1) for tu, tv in sel]
        drv.ask("row_block_occupancy", ntv, nu, W, *items_arg(items))
        drv.ask("touched_tiles", ntu * ntv, ntv, nu, nv, W, *items_arg(items))
    out = drv.run()
    for k, sel in enumerate(selections):
        cells = set().union(*(_footprint_cells(tu, tv, nu, nv, W) for tu, tv in sel))
        occ = [0] * ceil_div(nu, TP)
        touched = [0] * (ntu * ntv)
        for r, c in cells:
            occ[r // TP] = 1
            touched[(r // TILE) * ntv + c // TILE] = 1
        assert [int(x) for x in out[2 * k].split()] == occ, (grid, W, sel)
        assert [int(x) for x in out[2 * k + 1].split()] == touched, (grid, W, sel)


def test_short_last_block_is_run_through(drv):
    """nu = 40, W = 16: the footprints of tile row 0 run through the 8-row block 1 and wrap into block 0; those of tile row 1
    (rows 32 .. 39 + 46 wrapped) reach both as well"""
    drv.ask("row_block_occupancy", 2, 40, 16, *items_arg([(0, 0, 1)]))
    drv.ask("row_block_occupancy", 2, 40, 4, *items_arg([(0, 0, 1)]))
    drv.ask("touched_tiles", 4, 2, 40, 64, 16, 0)
    out = drv.run()
    assert out[0].split() == ["1", "1"] and out[1].split() == ["1", "1"] and out[2].split() == []


# ---- column_runs ------------------------------------------------------------------------------------------------------------
def test_column_runs(drv):
    nu, nv = 5 * TILE + 8, 7 * TILE + 5  # a short last tile row (8 rows) and a short last tile column (5 columns)
    ntu, ntv = 6, 8
    rows = ["00000000",   # no run
            "01110000",   # one
            "11000011",   # two, the second ends in the short column
            "10101000",   # three: the whole row
            "11111111",   # one run of everything
            "00010001"]   # the short tile row, two runs
    touched = [int(ch) for row in rows for ch in row]
    drv.ask("column_runs", nu, nv, ntv, *vec(touched))
    drv.ask("column_runs", nu, nv, ntv, 0)
    out = drv.run()
    tok = [int(x) for x in out[0].split()]
    cells, full, nruns = tok[:3]
    runs = [tuple(tok[3 + 4 * i:7 + 4 * i]) for i in range(nruns)]
    nrects = tok[3 + 4 * nruns]
    rects = [tuple(tok[4 + 4 * nruns + 4 * i:8 + 4 * nruns + 4 * i]) for i in range(nrects)]
    assert len(tok) == 4 + 4 * nruns + 4 * nrects and nruns == ntu
    covered = np.zeros((nu, nv), dtype=int)
    for row0, nr, col0, nc in rects:
        assert 0 < nr <= 8 and nc > 0 and row0 // TILE == (row0 + nr - 1) // TILE
        covered[row0:row0 + nr, col0:col0 + nc] += 1
    assert covered.max() == 1  # pairwise disjoint
    want = np.zeros((nu, nv), dtype=int)
    want_full, want_runs = 0, []
    for tu, row in enumerate(rows):
        r0, r1 = tu * TILE, min((tu + 1) * TILE, nu)
        rr = [(m.start() * TILE, min(m.end() * TILE, nv)) for m in re.finditer("1+", row)]
        if len(rr) >= 3:
            rr = [(0, nv)]
        for c0, c1 in rr:
            want[r0:r1, c0:c1] = 1
        want_full += (r1 - r0) * nv if rr else 0
        rr = (rr + [(0, 0), (0, 0)])[:2]
        want_runs.append(rr[0] + rr[1])
    assert np.array_equal(covered, want)
    # (the cells of the touched tiles, row by row -- or the whole row from three runs on)
    for tu, row in enumerate(rows):
        if len(re.findall("1+", row)) < 3:
            for tv, ch in enumerate(row):
                assert want[tu * TILE:(tu + 1) * TILE, tv * TILE:(tv + 1) * TILE].all() == (ch == "1")
    assert cells == int(want.sum()) and full == want_full and runs == want_runs
    # a plan without work: every tile row whole, no rectangles
    tok = [int(x) for x in out[1].split()]
    assert tok == [0, 0, ntu] + [0, nv, 0, 0] * ntu + [0]


# ---- occupied_spans ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occ,nu,spans,all_set", [
    ("0110010", 7 * 32, [(32, 64), (160, 32)], False),
    ("1101", 3 * 32 + 8, [(0, 64), (96, 8)], False),           # the last span is clipped to nu
    ("10101011", 8 * 32, [(0, 32), (64, 32), (128, 32), (192, 64)], False),  # four runs are kept
    ("101010101", 8 * 32 + 1, [(0, 8 * 32 + 1)], True),        # five: everything
    ("0000", 100, [], False),
])
def test_occupied_spans(drv, occ, nu, spans, all_set):
    drv.ask("occupied_spans", nu, *vec(int(c) for c in occ))
    tok = [int(x) for x in drv.run()[0].split()]
    n = tok[0]
    assert [(tok[1 + 2 * i], tok[2 + 2 * i]) for i in range(n)] == spans
    assert tok[1 + 2 * n:] == ([1] * len(occ) if all_set else [int(c) for c in occ])


# ---- xcd_row_map ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows", [63, 64, 200, 512])
def test_xcd_row_map(drv, nrows):
    spans = [(32, nrows // 3), (32 + nrows // 3 + 64, nrows - nrows // 3)]  # two spans with a gap
    rows = [r0 + i for r0, n in spans for i in range(n)]
    drv.ask("xcd_row_map", len(spans), *[x for s in spans for x in s])
    got = [int(x) for x in drv.run()[0].split()]
    assert sorted(got) == rows  # a permutation of the occupied rows
    nfull = nrows // 64
    for b in range(nrows):
        if b < nfull * 64:
            sg, r = divmod(b, 64)
            assert got[b] == rows[(sg * 8 + r % 8) * 8 + r // 8]
        else:
            assert got[b] == rows[b]


# ---- gather_chunk, scatter_chunk --------------------------------------------------------------------------------------------
def test_chunk_rules(drv):
    ns = [0, 1, 100000, 1000000, 4000000, 9500000, 20000000, 100000000]
    asks = [(wmode, n, col) for wmode in (0, 1, 2) for n in ns for col in (0, 1)]
    for a in asks:
        drv.ask("chunks", *a)
    out = [tuple(int(x) for x in line.split()) for line in drv.run()]
    res = dict(zip(asks, out))
    for (wmode, n, col), (gc, sc) in res.items():
        if wmode != 2:
            assert (gc, sc) == (CHUNK, CHUNK)
            continue
        # about three items per slot of 768 (and per launch): the smallest power of two from 512 with 1.5 c >= n / (3 * 768)
        want_g = next(c for c in (512, 1024, 2048, 4096) if c == 4096 or c * 1.5 >= n / (3.0 * 768.0))
        per_launch = n / (4.0 if col else 1.0)
        want_s = min(want_g, next(c for c in (512, 1024, 2048) if c == 2048 or c * 1.5 >= per_launch / (3.0 * 768.0)))
        assert (gc, sc) == (want_g, want_s), (n, col)
        assert gc in (512, 1024, 2048, 4096) and sc in (512, 1024, 2048) and sc <= gc
    for col in (0, 1):
        seq = [res[2, n, col] for n in ns]
        assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(seq, seq[1:]))  # non-decreasing in nactive
    assert res[2, 4000000, 1] == (2048, 512) and res[2, 100000000, 0] == (4096, 2048) and res[2, 0, 0] == (512, 512)


# ---- wd_derivative_table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,W,D1", [(1, 4, 13), (2, 16, 13), (4, 7, 13), (4, 5, 3)])
def test_wd_derivative_table(drv, K, W, D1):
    rng = np.random.default_rng(K * 100 + W)
    ktab = rng.standard_normal(W * D1)
    drv.ask("wd_derivative_table", K, W, D1, W * D1, *[repr(float(x)) for x in ktab])
    got = np.array([float(x) for x in drv.run()[0].split()]).reshape(K, W, D1)
    assert np.array_equal(got[0], ktab.reshape(W, D1))
    for k in range(1, K):
        for a in range(W):
            d2 = np.polynomial.polynomial.polyder(got[k - 1, a], 2) * float(W) ** 2  # monomial coefficients, lowest first
            want = np.zeros(D1)
            want[:len(d2)] = d2 if D1 > 2 else 0.0
            # (three roundings on either side, in a different order: a few units of 1.1e-16)
            np.testing.assert_allclose(got[k, a], want, rtol=1e-15, atol=0)
    assert math.isfinite(got.sum())
