// asan_planfile.cpp -- the plan-file validator under AddressSanitizer / UBSan, on the host alone.
//
// Built from cfs_planfile.hpp and cfs_plan.hpp only (tests/test_planfile_sanitized.py compiles and runs
// it): writes the plan of a small banded matrix, then hands the validator every truncation length, a
// few thousand seeded byte flips and every size field overwritten with huge, negative and off-by-one
// values -- once as they are (the header checksum is then wrong too) and once with the header
// checksum recomputed, so that the size checks themselves are what stands between the value and the
// reads.  Every call must return; a damaged file must be refused; the program exits 0.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "cfs_planfile.hpp"

namespace pf = cfs_planfile;

// the validator over the first `len` bytes of a copy of `b` that is exactly `len` bytes long (so that a
// read past the end is a read past an allocation)
static int check_mem(const std::vector<unsigned char> &b, std::string &err, size_t len = (size_t)-1) {
  if (len > b.size()) len = b.size();
  if (len == 0) return pf::kErrFile; // (fmemopen takes no empty buffer; the empty file is checked through a real one)
  std::unique_ptr<unsigned char[]> c(new unsigned char[len]);
  memcpy(c.get(), b.data(), len);
  FILE *f = fmemopen(c.get(), len, "rb");
  if (!f) abort();
  static pf::Parsed P;
  err.clear();
  int rc = pf::parse_file(f, len, P, err);
  if (!rc) rc = pf::verify_sections(f, P, err);
  fclose(f);
  return rc;
}

#define REQUIRE(cond)                                                   \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "line %d: %s failed (%s)\n", __LINE__, #cond, err.c_str()); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const std::string path = dir + "/banded.plan";
  std::string err;
  // a banded symmetric matrix: n rows, half bandwidth 5, full CSR
  const int n = 70, band = 5;
  std::vector<int> rp(1, 0), ci;
  std::vector<double> va;
  for (int i = 0; i < n; i++) {
    for (int j = std::max(0, i - band); j <= std::min(n - 1, i + band); j++) {
      ci.push_back(j);
      va.push_back(i == j ? 20.0 : -1.0 / (1 + std::abs(i - j)));
    }
    rp.push_back((int)ci.size());
  }
  cfs_plan::Options opt;
  opt.keep_value_map = true;
  cfs_plan::SymPlan<double> P;
  if (!cfs_plan::build_plan<double>(n, rp.data(), ci.data(), va.data(), 1, 0, nullptr, opt, P)) {
    fprintf(stderr, "build_plan: %s\n", P.error.c_str());
    return 1;
  }
  pf::Extras x;
  x.nnz_caller = rp[n];
  REQUIRE(pf::save_plan(P, x, path.c_str(), "asan", err));
  {
    static pf::Parsed F;
    REQUIRE(pf::check_file(path.c_str(), F, err) == 0);
    REQUIRE(F.h.s.n == n && std::string(F.h.tag) == "asan");
  }
  std::vector<unsigned char> good;
  {
    FILE *f = fopen(path.c_str(), "rb");
    REQUIRE(f != nullptr);
    unsigned char buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) good.insert(good.end(), buf, buf + k);
    fclose(f);
  }
  REQUIRE(check_mem(good, err) == 0);
  long calls = 0;
  // every truncation length
  for (size_t len = 0; len < good.size(); len++, calls++) {
    REQUIRE(check_mem(good, err, len) == pf::kErrFile);
  }
  { // ... and the empty file, a directory and a missing path through the real entry
    static pf::Parsed F;
    const std::string empty = dir + "/empty.plan";
    FILE *f = fopen(empty.c_str(), "wb");
    REQUIRE(f != nullptr);
    fclose(f);
    REQUIRE(pf::check_file(empty.c_str(), F, err) == pf::kErrFile);
    REQUIRE(pf::check_file(dir.c_str(), F, err) == pf::kErrFile);
    REQUIRE(pf::check_file((dir + "/missing.plan").c_str(), F, err) == pf::kErrFile);
  }
  // seeded byte flips: half of them in the header and the table, where the sizes live
  uint64_t seed = 0x243F6A8885A308D3ull;
  auto rnd = [&]() {
    seed ^= seed << 13, seed ^= seed >> 7, seed ^= seed << 17;
    return seed;
  };
  for (int it = 0; it < 4000; it++, calls++) {
    std::vector<unsigned char> b = good;
    const size_t span = (it & 1) ? b.size() : (size_t)pf::kTableEnd;
    const size_t pos = rnd() % span;
    b[pos] ^= (unsigned char)(1u << (rnd() % 8));
    bool covered = pos < pf::kTableEnd; // (the zero padding between sections belongs to no checksum)
    for (uint32_t i = 0; i < pf::kSections; i++) {
      pf::Row r;
      memcpy(&r, good.data() + sizeof(pf::Header) + sizeof(pf::Row) * i, sizeof r);
      covered = covered || (pos >= r.offset && pos < r.offset + r.bytes);
    }
    const int rc = check_mem(b, err);
    REQUIRE(rc == pf::kErrFile || (!covered && rc == 0));
  }
  // size fields: file_bytes / payload_bytes, every scalar, offset and length of every table row
  std::vector<size_t> fields = {offsetof(pf::Header, file_bytes), offsetof(pf::Header, payload_bytes)};
  for (int k = 0; k < pf::kNumScalars; k++) fields.push_back(offsetof(pf::Header, s) + 8 * (size_t)k);
  for (uint32_t i = 0; i < pf::kSections; i++) {
    fields.push_back(sizeof(pf::Header) + 32 * (size_t)i + offsetof(pf::Row, offset));
    fields.push_back(sizeof(pf::Header) + 32 * (size_t)i + offsetof(pf::Row, bytes));
  }
  for (size_t fo : fields) {
    uint64_t orig;
    memcpy(&orig, good.data() + fo, 8);
    const uint64_t vals[] = {~0ull, 0x7fffffffffffffffull, 0x8000000000000000ull, (1ull << 40) + 1, 1ull << 40, 1ull << 32,
                             0xffffffffull, orig + 1, orig - 1, orig + 64, orig * 2 + 8, 0};
    for (uint64_t v : vals) {
      if (v == orig) continue;
      for (int fix = 0; fix < 2; fix++, calls++) {
        std::vector<unsigned char> b = good;
        memcpy(b.data() + fo, &v, 8);
        if (fix) { // a consistent header checksum: only the size checks and the section checksums are left
          pf::Header h;
          memcpy(&h, b.data(), sizeof h);
          h.head_sum = pf::head_checksum(h, (const pf::Row *)(b.data() + sizeof(pf::Header)));
          memcpy(b.data(), &h, sizeof h);
        }
        const int rc = check_mem(b, err);
        REQUIRE(rc == pf::kErrFile || (fix && rc == 0));
      }
    }
  }
  // 32-bit fields of the fixed part and of the rows (element sizes, ids)
  for (size_t fo = 8; fo < 40; fo += 4)
    for (uint32_t v : {0u, 1u, 0xffffffffu, 0x80000000u}) {
      std::vector<unsigned char> b = good;
      uint32_t o;
      memcpy(&o, b.data() + fo, 4);
      if (o == v) continue;
      memcpy(b.data() + fo, &v, 4);
      calls++;
      REQUIRE(check_mem(b, err) == pf::kErrFile);
    }
  printf("asan_planfile: %ld validator calls on a file of %zu bytes, all returned\n", calls, good.size());
  return 0;
}
