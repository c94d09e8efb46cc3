// cfs_planfile.hpp -- one tuned symmetric handle as a file: format, checksum, writer, validator.
//
// Host-only (no HIP include: g++ alone compiles it, with cfs_plan.hpp for the struct layouts).
// cfs_hip.hip adds the device side: cfs_hip_sym_save / cfs_hip_sym_load and the checksum kernel,
// which evaluates the SAME function (mix64 / checksum below) over the device arrays.
//
// Layout (little-endian, every offset a multiple of 64 bytes):
//
//   [0, sizeof(Header))                 Header: magic, version, struct sizes, every scalar of the
//                                       handle (Scalars), the kept choices, tag, plan_note
//   [sizeof(Header), + 32 * nsections)  section table: one Row {id, element bytes, offset, byte
//                                       length, checksum} per section, in id order
//   payload                             the sections in id order, zero-padded to 64 bytes; an absent
//                                       array is a zero-length section
//
// Sections 0 .. kHostFirst-1 are the device arrays of a SymMatrix<V> over their FULL allocated length
// (so that a loaded handle reports the same device_bytes), the rest the small host arrays that
// finish_setup(), stats() and the shard entry points read after create.  Not stored: the strip, the
// launch-slot tables (gfirst / group ranges) and the receive fold -- finish_setup() and set_recv()
// rebuild them -- and the timing-only ablation mode.
//
// Checksum of a byte range: split it into 64-bit little-endian words w_0 .. w_{m-1} (the tail
// zero-padded), and
//
//     checksum = sum_i mix64(w_i + (i + 1) * 0x9E3779B97F4A7C15)      (mod 2^64)
//     mix64(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//                z = (z ^ (z >> 27)) * 0x94D049BB133111EB
//                z =  z ^ (z >> 31)                                    (the splitmix64 finaliser)
//
// The word index enters the mixed value, so swapping two different words changes the sum; the sum
// itself is an associative and commutative integer sum, so it can be taken in any order, in pieces and
// in parallel, with the same bits on the host and on the GPU.  Header::head_sum is this function over
// the header (with head_sum = 0) followed by the section table.
//
// The checksum guards against truncated, damaged and mixed-up files.  It is not a MAC: a file whose
// checksums pass is TRUSTED input (its indices are not re-validated against each other), and the cache
// built on it is not a security boundary.
#pragma once

#include <sys/stat.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cfs_plan.hpp"

#if defined(__HIPCC__)
#define CFS_PF_HD __host__ __device__
#else
#define CFS_PF_HD
#endif

namespace cfs_planfile {

constexpr int kErrFile = -7; // CFS_HIP_ERR_FILE
constexpr uint64_t kMagic = 0x004e414c50534643ull; // "CFSPLAN\0"
constexpr uint32_t kVersion = 1;
constexpr int kTagMax = 255;

CFS_PF_HD inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the term of word `w` at word index `i`
CFS_PF_HD inline uint64_t word_term(uint64_t w, uint64_t i) { return mix64(w + (i + 1) * 0x9E3779B97F4A7C15ull); }

// checksum of `bytes` bytes that start at word index `first_word` of their range (a range is summed in
// pieces by adding the pieces' values; every piece but the last must be a multiple of 8 bytes long)
inline uint64_t checksum(const void *p, size_t bytes, uint64_t first_word = 0) {
  const unsigned char *b = (const unsigned char *)p;
  uint64_t s = 0, i = first_word;
  size_t k = 0;
  for (; k + 8 <= bytes; k += 8, i++) {
    uint64_t w;
    memcpy(&w, b + k, 8);
    s += word_term(w, i);
  }
  if (k < bytes) {
    uint64_t w = 0;
    memcpy(&w, b + k, bytes - k);
    s += word_term(w, i);
  }
  return s;
}

enum Section : uint32_t {
  // device arrays
  S_TILES = 0, S_SLOT_COL, S_ROWINFO, S_DIAG, S_SLICE_META, S_LEADLANE, S_VALS, S_SLOTS,
  S_CVALS, S_CROWS, S_CCOLS, S_FVALS, S_FROWS, S_FCOLS,
  S_VAL_MAP, S_CVAL_MAP, S_FVAL_MAP, S_DIAG_MAP,
  S_FOLD_REC, S_FOLD_IDX, S_SEND_PTR, S_SEND_IDX, S_SLOT_EXP,
  // host arrays
  S_GROUP_FIRST, S_GROUP_PTR, S_LAUNCH_ORDER, S_FOLD_DST, S_SEND_ROW, S_SEND_COUNTS, S_TILE_ROUNDS, S_ROW_SPLITS,
  kSections
};
constexpr uint32_t kHostFirst = S_GROUP_FIRST;
inline const char *section_name(uint32_t id) {
  static const char *const names[kSections] = {
      "tiles", "slot_col", "rowinfo", "diag", "slice_meta", "leadlane", "vals", "slots", "cvals", "crows", "ccols",
      "fvals", "frows", "fcols", "val_map", "cval_map", "fval_map", "diag_map", "fold_rec", "fold_idx", "send_ptr",
      "send_idx", "slot_exp", "group_first", "group_ptr", "launch_order", "fold_dst", "send_row", "send_counts",
      "tile_rounds", "row_splits"};
  return id < kSections ? names[id] : "?";
}

struct FoldRec { // what cfs_fold_kernel reads: {dst, e0, e1, e2 | -(offset + 2)}
  int32_t dst, e0, e1, e2;
};
static_assert(sizeof(FoldRec) == 16, "FoldRec must stay 16 bytes");

// fold records and the remainder lists [count, entries 2..] of destinations with more than three
// contributions (see cfs_fold_kernel); `mk(dst, e0, e1, e2)` builds a record
template <class Rec, class Make>
inline void make_fold_records(const std::vector<int32_t> &dst, const std::vector<int32_t> &ptr,
                              const std::vector<int32_t> &idx, std::vector<Rec> &rec, std::vector<int32_t> &rest,
                              Make mk) {
  rec.assign(dst.size() + 1, mk(0, 0, -1, -1));
  rest.clear();
  for (size_t i = 0; i < dst.size(); i++) {
    const int b = ptr[i], len = ptr[i + 1] - ptr[i];
    int e2 = len == 3 ? idx[b + 2] : -1;
    if (len > 3) {
      e2 = -((int)rest.size() + 2);
      rest.push_back(len - 2);
      rest.insert(rest.end(), idx.begin() + b + 2, idx.begin() + b + len);
    }
    rec[i] = mk(dst[i], idx[b], len > 1 ? idx[b + 1] : -1, e2);
  }
}

// every scalar needed to rebuild the handle (all 64-bit: no padding, one rule for the range check)
struct Scalars {
  int64_t n, row_begin, row_end, nranks, rank;
  int64_t flags; // cfs_hip_options.flags the schedule was built with (ablation bits cleared)
  int64_t max_slots, block_threads, lds_slots, wg_per_cu, num_cus, deterministic, mirrored;
  int64_t ngroups, ntiles, nslots, nvrows, nslices; // nslots / nvrows: sums over the tiles
  int64_t nhalo, onesided_slots;
  int64_t stream_len, slot_len, coo_len, coo_entries, far_len, far_entries, far_candidates;
  int64_t chained_packets, lane_packets, mirror_entries;
  int64_t nnz_low, nnz_diag, nnz_full, nnz_caller, has_value_map;
  int64_t nfold, nsend;
  int64_t n_group_first, n_group_ptr, n_launch_order, n_tile_rounds, n_row_splits, n_send_counts;
  int64_t combine, nt_stream, device_built; // the choices tune() kept
};
constexpr int kNumScalars = (int)(sizeof(Scalars) / 8);

struct Header {
  uint64_t magic;
  uint32_t version, header_bytes;
  uint32_t value_bytes, tile_bytes, slice_meta_bytes, fold_rec_bytes;
  uint32_t nsections, row_bytes;
  uint64_t file_bytes, payload_bytes;
  uint64_t head_sum;
  Scalars s;
  char tag[kTagMax + 1];
  char plan_note[256];
};
struct Row {
  uint32_t id, elem;
  uint64_t offset, bytes, sum;
};
static_assert(sizeof(Row) == 32, "Row must stay 32 bytes");
static_assert(sizeof(Header) == 64 + 8 * kNumScalars + 512, "Header must have no padding");
constexpr uint64_t kTableEnd = sizeof(Header) + (uint64_t)kSections * sizeof(Row);
inline uint64_t align64(uint64_t v) { return (v + 63) & ~(uint64_t)63; }

struct Parsed {
  Header h;
  Row rows[kSections];
};

inline uint64_t head_checksum(const Header &h, const Row *rows) {
  Header c = h;
  c.head_sum = 0;
  const uint64_t a = checksum(&c, sizeof c);
  return a + checksum(rows, sizeof(Row) * kSections, (sizeof c + 7) / 8);
}

// ---------------------------------------------------------------------------------------------
// what the header's counts say about a section: element size, and the byte length it must have
// (`exact`) or must at least have (a device array may be allocated longer than its logical length)
// ---------------------------------------------------------------------------------------------
struct Expect {
  uint32_t elem = 1;
  uint64_t count = 0; // elements
  bool exact = false;
};
inline Expect expect(const Header &h, uint32_t id) {
  const Scalars &s = h.s;
  const uint32_t vb = h.value_bytes;
  const bool vm = s.has_value_map != 0;
  auto E = [](uint32_t elem, int64_t count, bool exact = false) {
    Expect e;
    e.elem = elem, e.count = (uint64_t)count, e.exact = exact;
    return e;
  };
  switch (id) {
  case S_TILES: return E(h.tile_bytes, s.ntiles, true);
  case S_SLOT_COL: return E(4, s.nslots);
  case S_ROWINFO: return E(4, s.nvrows);
  case S_DIAG: return E(vb, s.nvrows);
  case S_SLICE_META: return E(h.slice_meta_bytes, s.nslices);
  case S_LEADLANE: return E(1, s.nslices * 64);
  case S_VALS: return E(vb, s.stream_len);
  case S_SLOTS: return E(2, s.slot_len);
  case S_CVALS: return E(vb, s.coo_len);
  case S_CROWS: return E(2, s.coo_len);
  case S_CCOLS: return E(2, s.coo_len);
  case S_FVALS: return E(vb, s.far_len);
  case S_FROWS: return E(2, s.far_len);
  case S_FCOLS: return E(4, s.far_len);
  case S_VAL_MAP: return E(4, vm ? s.stream_len : 0);
  case S_CVAL_MAP: return E(4, vm ? s.coo_len : 0);
  case S_FVAL_MAP: return E(4, vm ? s.far_len : 0);
  case S_DIAG_MAP: return E(4, vm ? s.nvrows : 0);
  case S_FOLD_REC: return E(h.fold_rec_bytes, s.nfold > 0 ? s.nfold + 1 : 0);
  case S_FOLD_IDX: return E(4, 0);
  case S_SEND_PTR: return E(4, s.nsend > 0 ? s.nsend + 1 : 0);
  case S_SEND_IDX: return E(4, 0);
  case S_SLOT_EXP: return E(2, s.deterministic ? s.nslots : 0);
  case S_GROUP_FIRST: return E(h.tile_bytes, s.n_group_first, true);
  case S_GROUP_PTR: return E(4, s.n_group_ptr, true);
  case S_LAUNCH_ORDER: return E(4, s.n_launch_order, true);
  case S_FOLD_DST: return E(4, s.nfold, true);
  case S_SEND_ROW: return E(4, s.nsend, true);
  case S_SEND_COUNTS: return E(4, s.n_send_counts, true);
  case S_TILE_ROUNDS: return E(4, s.n_tile_rounds, true);
  case S_ROW_SPLITS: return E(4, s.n_row_splits, true);
  default: return Expect();
  }
}

// steps 1-3 of the validator and the header checksum; reads only the header and the section table.
// Nothing is allocated from a size of the file; every product is taken with overflow detection.
inline int parse_file(FILE *f, uint64_t fsize, Parsed &P, std::string &err) {
  Header &h = P.h;
  if (fsize < sizeof(Header)) {
    err = "truncated: " + std::to_string(fsize) + " bytes, a plan file header has " + std::to_string(sizeof(Header));
    return kErrFile;
  }
  if (fseek(f, 0, SEEK_SET) != 0 || fread(&h, sizeof h, 1, f) != 1) {
    err = "cannot read the header";
    return kErrFile;
  }
  // (1) magic, version, struct sizes
  if (h.magic != kMagic) {
    err = "not a plan file (bad magic)";
    return kErrFile;
  }
  if (h.version != kVersion) {
    err = "format version " + std::to_string(h.version) + ", this library reads version " + std::to_string(kVersion);
    return kErrFile;
  }
  if (h.header_bytes != sizeof(Header) || h.row_bytes != sizeof(Row) || h.nsections != kSections) {
    err = "header layout mismatch (header " + std::to_string(h.header_bytes) + " bytes, " + std::to_string(h.nsections) +
          " sections of " + std::to_string(h.row_bytes) + " bytes)";
    return kErrFile;
  }
  if (h.value_bytes != 4 && h.value_bytes != 8) {
    err = "value size " + std::to_string(h.value_bytes) + " is neither 4 nor 8";
    return kErrFile;
  }
  if (h.tile_bytes != sizeof(cfs_plan::Tile) || h.slice_meta_bytes != sizeof(cfs_plan::SliceMeta) ||
      h.fold_rec_bytes != sizeof(FoldRec)) {
    err = "struct layout mismatch: file has Tile " + std::to_string(h.tile_bytes) + ", slice meta " +
          std::to_string(h.slice_meta_bytes) + ", fold record " + std::to_string(h.fold_rec_bytes) + " bytes, this library " +
          std::to_string(sizeof(cfs_plan::Tile)) + " / " + std::to_string(sizeof(cfs_plan::SliceMeta)) + " / " +
          std::to_string(sizeof(FoldRec));
    return kErrFile;
  }
  // (2) the file size against the section table
  if (h.file_bytes != fsize) {
    err = "truncated or extended: header says " + std::to_string(h.file_bytes) + " bytes, the file has " + std::to_string(fsize);
    return kErrFile;
  }
  if (fsize < kTableEnd || fread(P.rows, sizeof(Row), kSections, f) != kSections) {
    err = "truncated inside the section table";
    return kErrFile;
  }
  uint64_t pos = align64(kTableEnd), payload = 0;
  for (uint32_t i = 0; i < kSections; i++) {
    const Row &r = P.rows[i];
    const std::string nm = std::string("section ") + section_name(i);
    if (r.id != i) {
      err = nm + ": table row holds id " + std::to_string(r.id);
      return kErrFile;
    }
    if (r.offset != pos || r.bytes > fsize || r.offset > fsize - r.bytes) {
      err = nm + ": offset " + std::to_string(r.offset) + " + " + std::to_string(r.bytes) + " bytes does not fit (expected offset " +
            std::to_string(pos) + ", file " + std::to_string(fsize) + " bytes)";
      return kErrFile;
    }
    pos = align64(r.offset + r.bytes); // (<= fsize + 63: no overflow)
    payload += r.bytes;
  }
  if (pos != fsize || payload != h.payload_bytes) {
    err = "section table ends at " + std::to_string(pos) + " with " + std::to_string(payload) + " payload bytes, header says " +
          std::to_string(fsize) + " / " + std::to_string(h.payload_bytes);
    return kErrFile;
  }
  // (3) every section length against the header's counts
  {
    const int64_t *sc = (const int64_t *)&h.s;
    for (int k = 0; k < kNumScalars; k++)
      if (sc[k] < 0 || sc[k] > ((int64_t)1 << 40)) {
        err = "header scalar " + std::to_string(k) + " out of range: " + std::to_string(sc[k]);
        return kErrFile;
      }
    const Scalars &s = h.s;
    const int64_t i31 = 0x7fffffff;
    if (s.n > i31 || s.row_begin > s.row_end || s.row_end > s.n || s.nranks < 1 || s.nranks > 65536 || s.rank >= s.nranks ||
        s.ntiles > i31 || s.ngroups > i31 || s.nfold > i31 || s.nsend > i31 || s.lds_slots > 65536 || s.nslices > i31) {
      err = "header: problem size or rank out of range";
      return kErrFile;
    }
    if ((s.block_threads != 256 && s.block_threads != 512 && s.block_threads != 1024) || s.lds_slots % 64 != 0) {
      err = "header: block of " + std::to_string(s.block_threads) + " threads / window of " + std::to_string(s.lds_slots) + " slots";
      return kErrFile;
    }
    const bool groups_ok = s.n_group_ptr == s.n_group_first + 1 || (s.n_group_first == 0 && s.n_group_ptr == 0);
    if (!groups_ok || (s.n_group_first != s.ngroups && s.ntiles > 0) ||
        (s.n_launch_order != 0 && s.n_launch_order != s.n_group_first) || (s.n_tile_rounds != 0 && s.n_tile_rounds != s.ntiles) ||
        (s.n_row_splits != 0 && s.n_row_splits != s.nranks + 1) || (s.n_send_counts != 0 && s.n_send_counts != s.nranks)) {
      err = "header: group / rank table counts do not agree";
      return kErrFile;
    }
  }
  for (uint32_t i = 0; i < kSections; i++) {
    const Row &r = P.rows[i];
    const Expect e = expect(h, i);
    uint64_t need = 0;
    if (__builtin_mul_overflow(e.count, (uint64_t)e.elem, &need)) {
      err = std::string("section ") + section_name(i) + ": expected length overflows";
      return kErrFile;
    }
    if (r.elem != e.elem || r.bytes % e.elem != 0 || (e.exact ? r.bytes != need : r.bytes < need)) {
      err = std::string("section ") + section_name(i) + ": " + std::to_string(r.bytes) + " bytes of " + std::to_string(r.elem) +
            "-byte elements, the header's counts need " + (e.exact ? "exactly " : "at least ") + std::to_string(need) + " of " +
            std::to_string(e.elem);
      return kErrFile;
    }
  }
  // (4, first part) the checksum of the header and the table
  if (head_checksum(h, P.rows) != h.head_sum) {
    err = "checksum mismatch in the header / section table";
    return kErrFile;
  }
  h.tag[kTagMax] = 0;
  h.plan_note[255] = 0;
  return 0;
}

// step 4: the checksum of every section, streamed through a fixed buffer
inline int verify_sections(FILE *f, const Parsed &P, std::string &err) {
  std::vector<unsigned char> buf((size_t)1 << 20);
  for (uint32_t i = 0; i < kSections; i++) {
    const Row &r = P.rows[i];
    if (r.bytes == 0) {
      if (r.sum != 0) {
        err = std::string("checksum mismatch in section ") + section_name(i);
        return kErrFile;
      }
      continue;
    }
    if (fseek(f, (long)r.offset, SEEK_SET) != 0) {
      err = std::string("cannot seek to section ") + section_name(i);
      return kErrFile;
    }
    uint64_t sum = 0, done = 0;
    while (done < r.bytes) {
      const size_t len = (size_t)std::min<uint64_t>(buf.size(), r.bytes - done);
      if (fread(buf.data(), 1, len, f) != len) {
        err = std::string("cannot read section ") + section_name(i);
        return kErrFile;
      }
      sum += checksum(buf.data(), len, done / 8);
      done += len;
    }
    if (sum != r.sum) {
      err = std::string("checksum mismatch in section ") + section_name(i);
      return kErrFile;
    }
  }
  return 0;
}

// open a regular file for reading and report its size
inline FILE *open_plan(const char *path, uint64_t *fsize, std::string &err) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    err = std::string("cannot open ") + path + ": " + strerror(errno);
    return nullptr;
  }
  struct stat st;
  if (fstat(fileno(f), &st) != 0 || !S_ISREG(st.st_mode)) {
    err = std::string("cannot open ") + path + ": not a regular file";
    fclose(f);
    return nullptr;
  }
  *fsize = (uint64_t)st.st_size;
  return f;
}

// the validator: needs nothing but the file
inline int check_file(const char *path, Parsed &P, std::string &err) {
  uint64_t fsize = 0;
  FILE *f = open_plan(path, &fsize, err);
  if (!f) return kErrFile;
  int rc = parse_file(f, fsize, P, err);
  if (!rc) rc = verify_sections(f, P, err);
  fclose(f);
  if (rc) err = std::string(path) + ": " + err;
  return rc;
}

// ---------------------------------------------------------------------------------------------
// writer: path + ".tmp", renamed once complete.  The section lengths are known up front; the
// payload is appended in id order, the header and the table (with the checksums) are written last.
// ---------------------------------------------------------------------------------------------
struct Writer {
  FILE *f = nullptr;
  std::string path, tmp, error;
  Parsed P;
  uint64_t pos = 0;
  ~Writer() {
    if (f) {
      fclose(f);
      remove(tmp.c_str());
    }
  }
  bool fail(const std::string &what) {
    error = what + " " + tmp + ": " + strerror(errno);
    return false;
  }
  bool pad_to(uint64_t off) {
    static const char zeros[4096] = {0};
    while (pos < off) {
      const size_t len = (size_t)std::min<uint64_t>(sizeof zeros, off - pos);
      if (fwrite(zeros, 1, len, f) != len) return fail("cannot write");
      pos += len;
    }
    return true;
  }
  // `elem` / `bytes`: element size and byte length of every section
  bool begin(const char *path_, const Header &h, const uint32_t *elem, const uint64_t *bytes) {
    path = path_;
    tmp = path + ".tmp";
    P.h = h;
    uint64_t off = align64(kTableEnd), payload = 0;
    for (uint32_t i = 0; i < kSections; i++) {
      P.rows[i] = Row{i, elem[i], off, bytes[i], 0};
      off = align64(off + bytes[i]);
      payload += bytes[i];
    }
    P.h.file_bytes = off;
    P.h.payload_bytes = payload;
    f = fopen(tmp.c_str(), "wb");
    if (!f) return fail("cannot create");
    pos = 0;
    return pad_to(align64(kTableEnd));
  }
  // the bytes of section `id`, in pieces, in id order
  bool put(uint32_t id, const void *p, size_t len) {
    if (pos < P.rows[id].offset && !pad_to(P.rows[id].offset)) return false;
    if (len && fwrite(p, 1, len, f) != len) return fail("cannot write");
    pos += len;
    return true;
  }
  bool finish(const uint64_t *sums) {
    if (!pad_to(P.h.file_bytes)) return false;
    for (uint32_t i = 0; i < kSections; i++) P.rows[i].sum = sums[i];
    P.h.head_sum = head_checksum(P.h, P.rows);
    if (fseek(f, 0, SEEK_SET) != 0 || fwrite(&P.h, sizeof(Header), 1, f) != 1 ||
        fwrite(P.rows, sizeof(Row), kSections, f) != kSections || fflush(f) != 0)
      return fail("cannot write");
    FILE *g = f;
    f = nullptr;
    if (fclose(g) != 0) {
      remove(tmp.c_str());
      return fail("cannot close");
    }
    if (rename(tmp.c_str(), path.c_str()) != 0) {
      remove(tmp.c_str());
      return fail("cannot rename");
    }
    return true;
  }
};

// what a handle knows beyond its SymPlan
struct Extras {
  int flags = 0, num_cus = 0;
  int64_t nnz_caller = 0, nslices = 0;
  bool combine = false, nt_stream = false, device_built = false;
  std::string plan_note;
};

template <typename V>
inline void fill_header(const cfs_plan::SymPlan<V> &P, const Extras &x, const char *tag, bool has_value_map, Header &h) {
  memset(&h, 0, sizeof h);
  h.magic = kMagic;
  h.version = kVersion;
  h.header_bytes = sizeof(Header);
  h.value_bytes = sizeof(V);
  h.tile_bytes = sizeof(cfs_plan::Tile);
  h.slice_meta_bytes = sizeof(cfs_plan::SliceMeta);
  h.fold_rec_bytes = sizeof(FoldRec);
  h.nsections = kSections;
  h.row_bytes = sizeof(Row);
  Scalars &s = h.s;
  s.n = P.n, s.row_begin = P.row_begin, s.row_end = P.row_end, s.nranks = P.nranks, s.rank = P.rank;
  s.flags = x.flags & ~7;
  s.max_slots = P.max_slots, s.block_threads = P.block_threads, s.lds_slots = P.lds_slots, s.wg_per_cu = P.wg_per_cu;
  s.num_cus = x.num_cus, s.deterministic = P.deterministic, s.mirrored = P.mirrored;
  s.ngroups = P.ngroups, s.ntiles = (int64_t)P.tiles.size();
  for (const cfs_plan::Tile &t : P.tiles) s.nslots += t.nslots, s.nvrows += t.nvrows;
  s.nslices = x.nslices;
  s.nhalo = P.nhalo, s.onesided_slots = P.onesided_slots;
  s.stream_len = P.stream_len, s.slot_len = P.slot_len, s.coo_len = P.coo_len, s.coo_entries = P.coo_entries;
  s.far_len = P.far_len, s.far_entries = P.far_entries, s.far_candidates = P.far_candidates;
  s.chained_packets = P.chained_packets, s.lane_packets = P.lane_packets, s.mirror_entries = P.mirror_entries;
  s.nnz_low = P.nnz_low, s.nnz_diag = P.nnz_diag, s.nnz_full = P.nnz_full, s.nnz_caller = x.nnz_caller;
  s.has_value_map = has_value_map;
  s.nfold = (int64_t)P.fold_dst.size(), s.nsend = (int64_t)P.send_row.size();
  s.n_group_first = (int64_t)P.group_first.size(), s.n_group_ptr = (int64_t)P.group_ptr.size();
  s.n_launch_order = (int64_t)P.launch_order.size(), s.n_tile_rounds = (int64_t)P.tile_rounds.size();
  s.n_row_splits = (int64_t)P.row_splits.size(), s.n_send_counts = (int64_t)P.send_counts.size();
  s.combine = x.combine, s.nt_stream = x.nt_stream, s.device_built = x.device_built;
  snprintf(h.tag, sizeof h.tag, "%s", tag ? tag : "");
  snprintf(h.plan_note, sizeof h.plan_note, "%s", x.plan_note.c_str());
}

// the small host arrays of a plan (sections kHostFirst ..): pointer and byte length
template <typename V> inline void host_section(const cfs_plan::SymPlan<V> &P, uint32_t id, const void **p, uint64_t *bytes) {
  auto set = [&](const auto &v) {
    *p = v.data();
    *bytes = (uint64_t)v.size() * sizeof(v[0]);
  };
  switch (id) {
  case S_GROUP_FIRST: return set(P.group_first);
  case S_GROUP_PTR: return set(P.group_ptr);
  case S_LAUNCH_ORDER: return set(P.launch_order);
  case S_FOLD_DST: return set(P.fold_dst);
  case S_SEND_ROW: return set(P.send_row);
  case S_SEND_COUNTS: return set(P.send_counts);
  case S_TILE_ROUNDS: return set(P.tile_rounds);
  case S_ROW_SPLITS: return set(P.row_splits);
  default: *p = nullptr, *bytes = 0;
  }
}

// a plan that is still whole on the host (build_plan's result, before any upload) -> file, with the
// checksum in its host form.  Returns false with `err` set.
template <typename V>
inline bool save_plan(const cfs_plan::SymPlan<V> &P, Extras x, const char *path, const char *tag, std::string &err) {
  std::vector<FoldRec> rec;
  std::vector<int32_t> rest;
  make_fold_records(P.fold_dst, P.fold_ptr, P.fold_idx, rec, rest,
                    [](int a, int b, int c, int d) { return FoldRec{a, b, c, d}; });
  x.nslices = (int64_t)P.slice_meta.size();
  Header h;
  fill_header(P, x, tag, !P.val_map.empty(), h);
  const void *ptr[kSections];
  uint64_t bytes[kSections];
  uint32_t elem[kSections];
  auto set = [&](uint32_t id, const auto &v) {
    ptr[id] = v.data();
    bytes[id] = (uint64_t)v.size() * sizeof(v[0]);
  };
  set(S_TILES, P.tiles), set(S_SLOT_COL, P.slot_col), set(S_ROWINFO, P.rowinfo), set(S_DIAG, P.diag);
  set(S_SLICE_META, P.slice_meta), set(S_LEADLANE, P.leadlane), set(S_VALS, P.vals), set(S_SLOTS, P.slots);
  set(S_CVALS, P.cvals), set(S_CROWS, P.crows), set(S_CCOLS, P.ccols);
  set(S_FVALS, P.fvals), set(S_FROWS, P.frows), set(S_FCOLS, P.fcols);
  set(S_VAL_MAP, P.val_map), set(S_CVAL_MAP, P.cval_map), set(S_FVAL_MAP, P.fval_map), set(S_DIAG_MAP, P.diag_map);
  set(S_FOLD_REC, rec), set(S_FOLD_IDX, rest), set(S_SEND_PTR, P.send_ptr), set(S_SEND_IDX, P.send_idx);
  set(S_SLOT_EXP, P.slot_exp);
  if (!P.deterministic) bytes[S_SLOT_EXP] = 0;
  for (uint32_t id = kHostFirst; id < kSections; id++) host_section(P, id, &ptr[id], &bytes[id]);
  for (uint32_t id = 0; id < kSections; id++) elem[id] = expect(h, id).elem;
  Writer w;
  uint64_t sums[kSections];
  bool ok = w.begin(path, h, elem, bytes);
  for (uint32_t id = 0; ok && id < kSections; id++) {
    sums[id] = checksum(ptr[id], (size_t)bytes[id]);
    ok = w.put(id, ptr[id], (size_t)bytes[id]);
  }
  ok = ok && w.finish(sums);
  if (!ok) err = w.error;
  return ok;
}

} // namespace cfs_planfile
