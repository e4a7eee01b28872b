"""
The bookkeeping of the training stash reservation, csrc/stash_book.h, compiled by g++ into a program of its own and driven with
lines of commands: room in the reservation, ownership of a stashed pass across close / re-open / flush, and the arithmetic of
the flush's weight-gradient GEMM for every set of contributors.
"""
import itertools
import os

import pytest

from host_tools import CSRC, host_header_program

HOST_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "stash_book.h"
using namespace pny;
// one command per line; every query prints one line
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 3;
    StashBook book;
    std::vector<StashedPass> passes(1);   // [0]: a pass no forward ever stashed
    char cmd[32];
    long long a, b, c;
    while (fscanf(f, "%31s", cmd) == 1) {
        if (!strcmp(cmd, "open")) {            // open ns coarse_tiles fine_tiles
            if (fscanf(f, "%lld %lld %lld", &a, &b, &c) != 3) return 4;
            const long long tiles[2] = {b, c};
            book.open((int)a, tiles);
        } else if (!strcmp(cmd, "close")) {
            book.close();
        } else if (!strcmp(cmd, "room")) {     // room which ns tiles
            if (fscanf(f, "%lld %lld %lld", &a, &b, &c) != 3) return 4;
            printf("%d\n", book.has_room((int)a, (int)b, c) ? 1 : 0);
        } else if (!strcmp(cmd, "take")) {     // take which tiles: the first tile
            if (fscanf(f, "%lld %lld", &a, &b) != 2) return 4;
            printf("%lld\n", book.take((int)a, b));
        } else if (!strcmp(cmd, "pass")) {     // pass which tiles n_points: remembered; its number, first tile and tile count
            if (fscanf(f, "%lld %lld %lld", &a, &b, &c) != 3) return 4;
            passes.push_back(book.take_pass((int)a, b, c));
            const StashedPass& sp = passes.back();
            printf("%d %d %lld %lld %lld %d\n", (int)passes.size() - 1, sp.which, sp.tile0, sp.tiles, sp.n_points, sp.valid ? 1 : 0);
        } else if (!strcmp(cmd, "owns")) {     // owns pass_number
            if (fscanf(f, "%lld", &a) != 1) return 4;
            printf("%d\n", book.owns(passes[(size_t)a]) ? 1 : 0);
        } else if (!strcmp(cmd, "note")) {     // note precision_code
            if (fscanf(f, "%lld", &a) != 1) return 4;
            book.note_contributor((Prec)a);
        } else if (!strcmp(cmd, "gemm")) {     // gemm have_absmax
            if (fscanf(f, "%lld", &a) != 1) return 4;
            printf("%d\n", (int)book.flush_gemm(a != 0));
        } else if (!strcmp(cmd, "flushed")) {  // flushed which clear_contributors
            if (fscanf(f, "%lld %lld", &a, &b) != 2) return 4;
            book.flushed((int)a, b != 0);
        } else if (!strcmp(cmd, "used")) {     // used which
            if (fscanf(f, "%lld", &a) != 1) return 4;
            printf("%lld\n", book.used[a]);
        } else {
            return 5;
        }
    }
    fclose(f);
    return 0;
}
"""

F32, H2, H1 = 0, 1, 2           # the codes of csrc/stash_book.h enum Prec (pny_model_last_flush_precision)
NS = 2


@pytest.fixture(scope="module")
def book(tmp_path_factory):
    """-> run(commands): the printed lines of a fresh StashBook driven by `commands`.  Nothing but <cstdint> under the header:
    no HIP include path, no defines."""
    program = host_header_program(tmp_path_factory.mktemp("stash_book_host"), HOST_MAIN, defines=(), include_dirs=(CSRC,),
                                  extra_flags=("-O1", "-Wall", "-Wextra", "-Werror"))
    return lambda commands: [line for line in program(commands) if line]


def test_header_includes_nothing_but_cstdint():
    with open(os.path.join(CSRC, "stash_book.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<cstdint>"]


def test_room_is_counted_per_mlp_and_per_view_count(book):
    got = book(["open %d 1 2" % NS, "room 0 %d 1" % NS, "take 0 1", "room 0 %d 1" % NS, "room 1 %d 2" % NS, "room 1 %d 3" % NS,
                "room 0 %d 0" % NS, "room 1 %d 2" % (NS + 1), "room 1 %d 2" % (NS - 1), "take 1 1", "take 1 1", "room 1 %d 1" % NS,
                "used 0", "used 1"])
    assert got == ["1", "0", "0", "1", "0",     # room for the one coarse tile; its first tile is 0; then none, the fine ones untouched
                   "1", "0", "0",               # (no tiles always fit); another view count has no room
                   "0", "1", "0", "1", "2"]     # consecutive tiles, then full


def test_pass_is_owned_until_close_or_reopen(book):
    got = book(["open %d 1 2" % NS, "pass 0 1 64", "pass 1 2 96", "owns 1", "owns 2", "owns 0",
                "close", "owns 1", "owns 2",
                "open %d 1 2" % NS, "owns 1", "owns 2", "pass 0 1 64", "owns 3",
                "close", "open %d 1 2" % NS, "owns 3"])
    assert got == ["1 0 0 1 64 1", "2 1 0 2 96 1", "1", "1", "0",     # (a pass nobody stashed is never owned)
                   "0", "0",                                           # not after close() ...
                   "0", "0", "3 0 0 1 64 1", "1",                      # ... nor in the next reservation, whose own pass is
                   "0"]                                                # and a close + open in one go (a new step) disowns it


def test_coarse_pass_survives_a_fine_only_flush(book):
    """PNYOLO_SPLIT_FLUSH: mlp_fine's flush runs between the scenes' fine and coarse backward passes."""
    got = book(["open %d 1 2" % NS, "pass 0 1 64", "pass 1 2 96", "used 0", "used 1",
                "flushed 1 0", "owns 1", "used 0", "used 1", "room 1 %d 2" % NS,
                "flushed 0 1", "used 0", "owns 1", "room 0 %d 1" % NS])
    assert got == ["1 0 0 1 64 1", "2 1 0 2 96 1", "1", "2",
                   "1", "1", "0", "1",          # still owned; mlp_fine's tiles are free again, mlp_coarse's are not
                   "0", "1", "1"]               # (the epoch does not change at a flush: ownership ends with the reservation)


# The flush's GEMM for every set of contributors, from the two places that decided it before the header existed.  A backward
# set defer_dw_f32 when its gradient GEMMs ran fp32 and defer_dw_h2 when they ran split f16 (single-plane ones set neither); the
# flush read  absmax = (the max |dY| words exist && !defer_dw_f32) ? word : null  and  gemm = !absmax ? fp32 : defer_dw_h2 ?
# split f16 : single-plane.  Keys: (an F32, a split-f16, a single-plane contributor, the words exist).
FLUSH_GEMM = {
    (0, 0, 0, 1): H1, (0, 0, 1, 1): H1, (0, 1, 0, 1): H2, (0, 1, 1, 1): H2,
    (1, 0, 0, 1): F32, (1, 0, 1, 1): F32, (1, 1, 0, 1): F32, (1, 1, 1, 1): F32,
    (0, 0, 0, 0): F32, (0, 0, 1, 0): F32, (0, 1, 0, 0): F32, (0, 1, 1, 0): F32,
    (1, 0, 0, 0): F32, (1, 0, 1, 0): F32, (1, 1, 0, 0): F32, (1, 1, 1, 0): F32,
}


def test_flush_gemm_for_every_set_of_contributors(book):
    assert set(FLUSH_GEMM) == set(itertools.product((0, 1), repeat=4))
    for (f32, h2, h1, have), want in sorted(FLUSH_GEMM.items()):
        notes = ["note %d" % code for code, on in ((H1, h1), (H2, h2), (F32, f32)) if on]
        for order in (notes, notes[::-1]):
            assert book(["open %d 1 2" % NS] + order + ["gemm %d" % have]) == [str(want)], (f32, h2, h1, have)


def test_contributors_are_cleared_by_a_flush_that_says_so(book):
    got = book(["open %d 1 2" % NS, "note %d" % F32, "note %d" % H2, "gemm 1",
                "flushed 1 0", "gemm 1",          # fine-only flush: the coarse-only one of the same step still sees them
                "flushed 0 1", "gemm 1",
                "note %d" % H2, "gemm 1", "flushed 0 0", "flushed 1 1", "gemm 1"])
    assert got == [str(F32), str(F32), str(H1), str(H2), str(H1)]


def test_closed_book_says_no(book):
    never, closed = ["room 0 %d 0" % NS, "room 0 0 0", "room 1 %d 1" % NS, "owns 0"], ["close", "owns 1", "room 0 %d 0" % NS, "room 1 %d 1" % NS]
    assert book(never) == ["0"] * 4
    assert book(["open %d 4 4" % NS, "pass 0 1 64"] + closed)[1:] == ["0"] * 3
    assert book(["open %d 4 4" % NS, "pass 0 1 64"] + closed + ["used 0", "used 1"])[-2:] == ["0", "0"]
