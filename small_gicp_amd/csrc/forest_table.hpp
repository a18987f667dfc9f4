// The layout of a batched chain's table (forest.hpp), stated once per table: the sections are declared in order,
// each starts on an 8-byte word and takes whole words, and a section's handle gives a typed pointer into any copy of the table — the
// staging slot the host fills, or the device buffer, whose addresses are known before anything is uploaded (members hold pointers into
// their own table).  Host-only and free of HIP, so that tests/cpp/test_forest_table.cpp checks it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace sga {

template <typename T>
struct TableSection {
  size_t word = 0, count = 0;  // first 8-byte word of the section; its elements
};

struct TableLayout {
  size_t words_ = 0;
  // `count` elements of T behind the sections declared so far.  The member array goes first: the kernels read it with scalar loads.
  template <typename T>
  TableSection<T> add(size_t count) {
    static_assert(alignof(T) <= 8, "a section starts on an 8-byte word");
    const TableSection<T> s{words_, count};
    words_ += (count * sizeof(T) + 7) / 8;
    return s;
  }
  // the prefix sums of `grids` launch grids over `count` members, count + 1 entries each, one behind the other (grid g starts at
  // entry g * (count + 1): the kernels receive plain pointers)
  TableSection<uint32_t> add_prefixes(size_t grids, size_t count) { return add<uint32_t>(grids * (count + 1)); }
  size_t words() const { return words_; }
  template <typename T>
  static T* at(const TableSection<T>& s, unsigned long long* base) {
    return reinterpret_cast<T*>(base + s.word);
  }
  // the section's elements copied from `src` into the table at `base`
  template <typename T>
  static void put(const TableSection<T>& s, unsigned long long* base, const T* src) {
    std::memcpy(base + s.word, src, s.count * sizeof(T));
  }
};

}  // namespace sga
