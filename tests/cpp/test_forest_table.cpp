// The layouts of the batched chains' tables (small_gicp_amd/csrc/forest_table.hpp), rebuilt section by section as the host code declares
// them, for 1, 2, 3 and 64 members: every section filled to its full extent with a byte pattern of its own in a buffer of exactly
// words() * 8 bytes.  No pattern may be disturbed, every section starts on an 8-byte word, and the sections cover the buffer one behind
// the other.  Built with -fsanitize=address,undefined (tests/test_forest_table.py): a section past the end of the buffer is an error there.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "forest_table.hpp"

using sga::TableLayout;
using sga::TableSection;

template <size_t N>
struct Rec {  // stands for a chain's member struct of N bytes (pointers and doubles: aligned to 8)
  alignas(8) unsigned char b[N];
};

struct Table {
  TableLayout L;
  struct Span {
    size_t word, bytes;
    std::function<unsigned char*(unsigned long long*)> at;
  };
  std::vector<Span> spans;
  template <typename T>
  Table& add(size_t count) {
    const TableSection<T> s = L.add<T>(count);
    spans.push_back({s.word, count * sizeof(T), [s](unsigned long long* base) { return reinterpret_cast<unsigned char*>(TableLayout::at(s, base)); }});
    return *this;
  }
  Table& prefixes(size_t grids, size_t count) {
    const TableSection<uint32_t> s = L.add_prefixes(grids, count);
    spans.push_back({s.word, grids * (count + 1) * sizeof(uint32_t), [s](unsigned long long* base) { return reinterpret_cast<unsigned char*>(TableLayout::at(s, base)); }});
    return *this;
  }
};

static int check(const char* name, size_t count, const Table& t) {
  int bad = 0;
  auto fail = [&](const char* what, size_t k) {
    std::printf("FAIL %s (%zu members): section %zu %s\n", name, count, k, what);
    bad++;
  };
  const size_t bytes = t.L.words() * 8;
  unsigned long long* base = static_cast<unsigned long long*>(std::malloc(bytes));
  for (size_t k = 0; k < t.spans.size(); k++) {
    unsigned char* p = t.spans[k].at(base);
    for (size_t i = 0; i < t.spans[k].bytes; i++) p[i] = static_cast<unsigned char>(k + 1);
  }
  size_t next = 0;  // the word the next section has to start on
  for (size_t k = 0; k < t.spans.size(); k++) {
    const Table::Span& s = t.spans[k];
    unsigned char* p = s.at(base);
    if (reinterpret_cast<uintptr_t>(p) % 8 != 0) fail("is not aligned to 8 bytes", k);
    if (p != reinterpret_cast<unsigned char*>(base + s.word)) fail("is not where its handle says", k);
    if (s.word != next) fail("does not start where the section before it ends", k);
    for (size_t i = 0; i < s.bytes; i++)
      if (p[i] != static_cast<unsigned char>(k + 1)) {
        fail("was overwritten by another section", k);
        break;
      }
    next = s.word + (s.bytes + 7) / 8;
  }
  if (next != t.L.words()) fail("(the last) does not end with the buffer", t.spans.size() - 1);
  std::free(base);
  return bad;
}

int main() {
  int bad = 0, tables = 0;
  for (size_t n : {size_t(1), size_t(2), size_t(3), size_t(64)}) {
    auto run = [&](const char* name, const Table& t) { bad += check(name, n, t), tables++; };
    // kd forest: [trees][tail accumulators: 4 words each][ticket][member lists: as many entries as the steps take]
    run("kd forest", Table().add<Rec<152>>(n).add<unsigned long long>(4 * n).add<unsigned>(1).add<uint32_t>(5 * n + 1));
    run("kd forest, even lists", Table().add<Rec<152>>(n).add<unsigned long long>(4 * n).add<unsigned>(1).add<uint32_t>(4 * n));
    run("features forest", Table().add<Rec<168>>(n).prefixes(2, n));
    run("grid forest", Table().add<Rec<136>>(n).add<uint32_t>(4 * n).add<unsigned>(1).prefixes(3, n));
    run("map build, table 1", Table().add<Rec<128>>(n).add<int>(6 * n).add<unsigned>(1).prefixes(1, n));
    run("map build, table 2", Table().add<Rec<128>>(n).prefixes(2, n));
    run("insert, table 1", Table().add<Rec<160>>(n).add<int>(6 * n).add<unsigned>(2 * n).add<unsigned>(1).prefixes(1, n));
    run("insert, table 2", Table().add<Rec<208>>(n).prefixes(1, n));
    run("insert, table 3", Table().add<Rec<64>>(n).prefixes(1, n));
    run("problem creation", Table().add<Rec<232>>(n).add<int>(6 * n).add<unsigned>(n).add<unsigned>(1).prefixes(1, n));
    run("cloud merge", Table().add<Rec<136>>(n).prefixes(1, n));
    run("cloud deskew", Table().add<Rec<192>>(n).prefixes(1, n).add<unsigned long long>(8 * n).add<unsigned>(1));
    run("cloud deskew, no boxes", Table().add<Rec<192>>(n).prefixes(1, n).add<unsigned long long>(0).add<unsigned>(1));
  }
  // put: a section's elements arrive where at() points, and nowhere else
  {
    TableLayout L;
    const auto a = L.add<uint32_t>(3);
    const auto b = L.add<uint32_t>(5);
    std::vector<unsigned long long> buf(L.words(), 0ull);
    const uint32_t src[5] = {1, 2, 3, 4, 5};
    TableLayout::put(b, buf.data(), src);
    for (size_t i = 0; i < 3; i++) bad += TableLayout::at(a, buf.data())[i] != 0u;
    for (size_t i = 0; i < 5; i++) bad += TableLayout::at(b, buf.data())[i] != src[i];
  }
  std::printf("%s: %d tables, %d failures\n", bad ? "FAILED" : "OK", tables, bad);
  return bad ? 1 : 0;
}
