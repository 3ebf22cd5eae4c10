"""RangeStore (strolle_amd/csrc/st_ranges.h) — the posed, bind and target stores of st_deform.cpp hand out their ranges through it — replayed on the
host under AddressSanitizer and UBSan: a few thousand random takes and gives against a plain model of the occupied intervals. No range
overlaps another or ends beyond the store's length, and every take returns the first index that bare SlotRanges with an append counter
beside it returns (which range a take returns decides device addresses)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "st_ranges.h"
#include <cstdio>
#include <cstdlib>
#include <random>

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s (op %d)\n", __LINE__, #c, op); return 1; } } while (0)

int main() {
    std::mt19937 rng(12345);
    for (int round = 0; round < 4; round++) {
        st::RangeStore store;
        st::SlotRanges bare; size_t bare_size = 0;            // what the callers wrote out by hand before
        std::vector<std::pair<size_t, size_t>> held;           // (first, n)
        const size_t longest = round % 2 ? 300u : 8u;          // (short ranges: many exact fits and merges)
        for (int op = 0; op < 3000; op++) {
            if (held.empty() || rng() % 100 < 55) {
                const size_t n = 1u + rng() % longest;
                size_t b, e;
                const bool reused = bare.take(n, &b, &e);
                if (!reused) { b = bare_size; bare_size += n; }
                bool appended = reused;
                const size_t first = store.take(n, &appended);
                CHECK(first == b); CHECK(appended == !reused); CHECK(store.size == bare_size); CHECK(first + n <= store.size);
                for (const auto& h : held) CHECK(first + n <= h.first || h.first + h.second <= first);
                held.push_back({first, n});
            } else if (rng() % 20 == 0) {
                store.give(SIZE_MAX, 1u + rng() % longest);     // a record that never had a range
            } else {
                const size_t i = rng() % held.size();
                store.give(held[i].first, held[i].second); bare.give(held[i].first, held[i].first + held[i].second);
                held[i] = held.back(); held.pop_back();
            }
        }
        int op = -1;
        CHECK(store.take(0x7fffffffu) == bare_size);           // nothing that large was given back: the store's end
    }
    std::puts("ok");
    return 0;
}
"""


def test_range_store_against_a_model_of_occupied_intervals(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    src = tmp_path / "ranges.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "ranges"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "strolle_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
