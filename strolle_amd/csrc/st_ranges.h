// st_ranges.h — the host engine's index allocators (st_engine.h "small containers"): no HIP in here, so that they can be exercised on their own
// (tests/test_range_store.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace st {

struct SlotRanges {  // utils/allocator.rs
    std::vector<std::pair<size_t, size_t>> free_; bool unsorted = false;
    void give(size_t b, size_t e) { if (!free_.empty()) unsorted |= b <= free_.back().second; free_.push_back({b, e}); }
    bool take(size_t len, size_t* b, size_t* e) {
        if (unsorted && !free_.empty()) {
            std::stable_sort(free_.begin(), free_.end(), [](const auto& l, const auto& r) { return l.first < r.first; });
            for (size_t i = 0; i + 1 < free_.size();) {
                if (free_[i].second == free_[i + 1].first) { free_[i].second = free_[i + 1].second; free_.erase(free_.begin() + i + 1); }
                else i++;
            }
        }
        unsorted = false;
        for (size_t i = 0; i < free_.size(); i++) {
            const size_t have = free_[i].second - free_[i].first;
            if (have < len) continue;
            *b = free_[i].first; *e = *b + len;
            if (have == len) free_.erase(free_.begin() + i); else free_[i].first += len;
            return true;
        }
        return false;
    }
};
// A store handed out in ranges: SlotRanges over the ranges given back, and the length handed out so far (what its allocation has to hold).
struct RangeStore {
    SlotRanges free; size_t size = 0;
    // the first index of `n`: a range given back (first fit) or the store's end, which then moves (*appended)
    size_t take(size_t n, bool* appended = nullptr) {
        size_t b, e;
        const bool reused = free.take(n, &b, &e);
        if (!reused) { b = size; size += n; }
        if (appended) *appended = !reused;
        return b;
    }
    void give(size_t first, size_t n) { if (first != SIZE_MAX) free.give(first, first + n); }   // (SIZE_MAX: it never had a range)
};

}  // namespace st
