// csr.cpp -- CSRMatrix<int,float> / CSRMatrix<int,double> over the C ABI
// (the reference instantiates the same two: src/csr.cpp:10-11).
//
// file ctor   ~ include/matrix/csr_matrix.tpp:8-111   (own parallel reader)
// array ctor  ~ :113-144  (no ownership)
// tune()      ~ :230-310  -> cfs_hip_sym_create_* / cfs_hip_csr_create_*,
//                            then frees the full CSR like compress_symmetry (:1700-1706)
// multiply    ~ spmv_fn   -> cfs_hip_sym_spmv / cfs_hip_csr_spmv
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <type_traits>

#include "cfs.hpp"
#include "cfs_hip.h"
#include "io/mmf.hpp"

namespace cfs {
namespace matrix {
namespace sparse {

static void fatal(const std::string &msg) {
  std::cout << "[ERROR]: " << msg << std::endl;
  exit(1);
}

static void require_gpu(Platform p) {
  if (p != Platform::gpu)
    fatal("this build of cfs-spmv runs the SpMV path on the GPU only: "
          "Platform::cpu is not provided (no CPU fallback)");
  if (cfs_hip_init(cfs::util::runtime::get_device()) != 0)
    fatal(std::string("cannot initialise the HIP device: ") + cfs_hip_last_error());
}

template <typename IndexT, typename ValueT>
CSRMatrix<IndexT, ValueT>::CSRMatrix(const std::string &filename, Platform platform,
                                     bool symmetric, bool hybrid)
    : platform_(platform), owns_data_(true), hybrid_(hybrid), tuned_(false),
      sym_handle_(nullptr), csr_handle_(nullptr), device_bytes_(0) {
  require_gpu(platform_);
  cfs::io::CsrArrays<IndexT, ValueT> a;
  std::string err;
  if (!cfs::io::LoadMmfCsr<IndexT, ValueT>(filename, a, err)) {
    std::cout << err << std::endl; // the reference prints the bare message
    exit(1);
  }
  symmetric_ = a.symmetric && symmetric; // csr_matrix.tpp:13-15
  source_ = filename;
  src_size_ = a.src_size;
  src_mtime_ns_ = a.src_mtime_ns;
#ifdef _LOG_INFO
  if (!symmetric)
    std::cout << "[INFO]: using CSR format to store the sparse matrix..." << std::endl;
  else if (!a.symmetric)
    std::cout << "[INFO]: matrix is not symmetric!\n[INFO]: rolling back to CSR format..."
              << std::endl;
  else
    std::cout << "[INFO]: using " << (hybrid ? "HYB" : "SSS")
              << " format to store the sparse matrix..." << std::endl;
#endif
  nrows_ = a.nrows;
  ncols_ = a.ncols;
  nnz_ = (int)a.nnz;
  nthreads_ = (int)get_num_threads();
  rowptr_ = (IndexT *)internal_alloc(((size_t)nrows_ + 1) * sizeof(IndexT), Platform::cpu);
  colind_ = (IndexT *)internal_alloc((size_t)nnz_ * sizeof(IndexT), Platform::cpu);
  values_ = (ValueT *)internal_alloc((size_t)nnz_ * sizeof(ValueT), Platform::cpu);
  std::copy(a.rowptr.begin(), a.rowptr.end(), rowptr_);
  std::copy(a.colind.begin(), a.colind.end(), colind_);
  std::copy(a.values.begin(), a.values.end(), values_);
}

template <typename IndexT, typename ValueT>
CSRMatrix<IndexT, ValueT>::CSRMatrix(IndexT *rowptr, IndexT *colind, ValueT *values,
                                     IndexT nrows, IndexT ncols, bool symmetric, bool hybrid,
                                     Platform platform)
    : platform_(platform), nrows_(nrows), ncols_(ncols), symmetric_(symmetric),
      owns_data_(false), hybrid_(hybrid), tuned_(false), rowptr_(rowptr), colind_(colind),
      values_(values), sym_handle_(nullptr), csr_handle_(nullptr), device_bytes_(0) {
  require_gpu(platform_);
  nnz_ = rowptr_[nrows];
  nthreads_ = (int)get_num_threads();
}

template <typename IndexT, typename ValueT> void CSRMatrix<IndexT, ValueT>::release_host_csr() {
  if (owns_data_) {
    internal_free(rowptr_, Platform::cpu);
    internal_free(colind_, Platform::cpu);
    internal_free(values_, Platform::cpu);
  }
  rowptr_ = colind_ = nullptr;
  values_ = nullptr;
}

template <typename IndexT, typename ValueT> CSRMatrix<IndexT, ValueT>::~CSRMatrix() {
  if (sym_handle_) cfs_hip_sym_destroy((cfs_hip_sym_t)sym_handle_);
  if (csr_handle_) cfs_hip_csr_destroy((cfs_hip_csr_t)csr_handle_);
  release_host_csr();
}

template <typename IndexT, typename ValueT> size_t CSRMatrix<IndexT, ValueT>::size() const {
  if (tuned_) return device_bytes_;
  return ((size_t)nrows_ + 1) * sizeof(IndexT) + (size_t)nnz_ * (sizeof(IndexT) + sizeof(ValueT));
}

template <typename IndexT, typename ValueT>
bool CSRMatrix<IndexT, ValueT>::tune(Kernel, Tuning t) {
  if (tuned_) return true;
  static_assert(std::is_same<IndexT, int>::value, "int indices only (src/csr.cpp:10-11)");
  int rc;
  bool use_sss = symmetric_;
  std::string plan_path, plan_tag; // non-empty: the plan cache applies to this tune()
  if (use_sss) {
#ifdef _LOG_INFO
    std::cout << "[INFO]: compressing for symmetry: MI355X tile schedule" << std::endl;
#endif
    cfs_hip_sym_t h = nullptr;
    // Tuning::Aggressive (the default, as in the reference) also measures the XCDs
    // and re-cuts the rows; Tuning::None builds the schedule once
    cfs_hip_options opt;
    memset(&opt, 0, sizeof opt);
    if (t == Tuning::None) opt.flags |= CFS_HIP_FLAG_NO_CALIBRATE;
    // Format::hyb (csr_matrix.tpp:312-401 in the reference): entries whose column a
    // tile uses only once leave the tile format (kept by both tiles, one-sided)
    if (hybrid_) opt.flags |= CFS_HIP_FLAG_HYB;
    const int ngpus = cfs::util::runtime::get_num_gpus();
    // Plan cache (one GPU, a matrix that came from a file): with CFS_PLAN_CACHE_DIR set to a writable
    // directory the tuned handle is kept as <dir>/<basename>.<f32|f64>.<none|aggr>[.hyb].plan and
    // loaded instead of tune() on later runs.  The tag -- the source file's size and mtime (the
    // .csrbin rule, src/mmf.cpp), the tuning level and the HYB setting -- must match; anything else
    // is ignored and rewritten.
    const char *cdir = getenv("CFS_PLAN_CACHE_DIR");
    if (cdir && *cdir && ngpus == 1 && !source_.empty() && src_size_ >= 0) {
      const size_t slash = source_.find_last_of('/');
      plan_path = std::string(cdir) + "/" + (slash == std::string::npos ? source_ : source_.substr(slash + 1)) +
                  (sizeof(ValueT) == 8 ? ".f64" : ".f32") + (t == Tuning::None ? ".none" : ".aggr") + (hybrid_ ? ".hyb" : "") +
                  ".plan";
      plan_tag = "size=" + std::to_string(src_size_) + " mtime_ns=" + std::to_string(src_mtime_ns_) +
                 " tuning=" + (t == Tuning::None ? "none" : "aggressive") + " hyb=" + (hybrid_ ? "1" : "0");
      if (cfs_hip_sym_load(plan_path.c_str(), plan_tag.c_str(), &h) == 0) {
        std::cout << "[INFO]: plan cache hit: " << plan_path << std::endl;
        sym_handle_ = h;
        cfs_hip_sym_stats st;
        cfs_hip_sym_get_stats(h, &st);
        device_bytes_ = (size_t)st.device_bytes;
        release_host_csr();
        tuned_ = true;
        return true;
      }
      std::cout << "[INFO]: plan cache miss (" << cfs_hip_last_error() << "): running tune()" << std::endl;
    }
    if (ngpus > 1) { // CFS_NUM_GPUS: one shard per GPU, one stream each, this thread drives them
      if (std::is_same<ValueT, double>::value)
        rc = cfs_hip_sym_create_multi_f64(nrows_, rowptr_, colind_, (const double *)values_, ngpus,
                                          nullptr, &opt, &h);
      else
        rc = cfs_hip_sym_create_multi_f32(nrows_, rowptr_, colind_, (const float *)values_, ngpus,
                                          nullptr, &opt, &h);
    } else if (std::is_same<ValueT, double>::value)
      rc = cfs_hip_sym_create_f64(nrows_, rowptr_, colind_, (const double *)values_, &opt, &h);
    else
      rc = cfs_hip_sym_create_f32(nrows_, rowptr_, colind_, (const float *)values_, &opt, &h);
    if (rc == CFS_HIP_ERR_UNSUPPORTED) {
      // a row with more stored columns than an LDS window holds: the symmetric
      // schedule does not apply; the full CSR is still here, so the general HIP
      // kernel computes the same product (slower, never wrong)
      std::cout << "[INFO]: " << cfs_hip_last_error()
                << " -- falling back to the general CSR kernel on the GPU" << std::endl;
      use_sss = false;
    } else if (rc != 0) {
      fatal(std::string("tune() failed: ") + cfs_hip_last_error());
    } else {
      sym_handle_ = h;
    }
  }
  // Tuning::Aggressive, one GPU: where the symmetric schedule may not pay -- a matrix without
  // locality (power-law graphs: hub columns make nearly every column of a tile a halo slot or a
  // far entry; profiles/r03_powerlaw_*: 3.6 x the algorithmic bytes cross the HBM interface) --
  // the general CSR kernel over both triangles is MEASURED against it on the caller's matrix and
  // the faster one is kept.  Candidates: halo slots + far entries beyond a quarter of the stored
  // nonzeros (FEM-like matrices: 1-5 %).  Reference knob of the kind: the format argument of
  // create() (sparse_matrix.tpp:13-24) -- here the measured choice inside Format::sss.
  if (use_sss && t == Tuning::Aggressive && cfs::util::runtime::get_num_gpus() == 1 &&
      getenv("CFS_NO_FORMAT_CHOICE") == nullptr) {
    cfs_hip_sym_stats st;
    cfs_hip_sym_get_stats((cfs_hip_sym_t)sym_handle_, &st);
    if ((st.halo_slots + st.far_entries) * 4 > st.nnz_low && st.nnz_low >= 100000) {
      cfs_hip_csr_t g = nullptr;
      if (std::is_same<ValueT, double>::value)
        rc = cfs_hip_csr_create_f64(nrows_, ncols_, rowptr_, colind_, (const double *)values_, &g);
      else
        rc = cfs_hip_csr_create_f32(nrows_, ncols_, rowptr_, colind_, (const float *)values_, &g);
      void *xd = nullptr, *yd = nullptr, *e0 = nullptr, *e1 = nullptr;
      float ms_sym = 0, ms_csr = 0;
      bool ok = rc == 0 && cfs_hip_alloc((size_t)ncols_ * sizeof(ValueT), CFS_HIP_MEM_DEVICE, &xd) == 0 &&
                cfs_hip_alloc((size_t)nrows_ * sizeof(ValueT), CFS_HIP_MEM_DEVICE, &yd) == 0 &&
                cfs_hip_memset(xd, 0x3f, (size_t)ncols_ * sizeof(ValueT)) == 0 && // small positive values
                cfs_hip_event_create(&e0) == 0 && cfs_hip_event_create(&e1) == 0;
      for (int which = 0; ok && which < 2; which++) {
        auto run = [&]() {
          return which == 0 ? cfs_hip_sym_spmv_async((cfs_hip_sym_t)sym_handle_, yd, xd, nullptr)
                            : cfs_hip_csr_spmv_async(g, yd, xd, nullptr);
        };
        for (int it = 0; ok && it < 3; it++) ok = run() == 0; // (the CSR handle picks its kernel form here)
        ok = ok && cfs_hip_event_record(e0, nullptr) == 0;
        for (int it = 0; ok && it < 5; it++) ok = run() == 0;
        ok = ok && cfs_hip_event_record(e1, nullptr) == 0 &&
             cfs_hip_event_elapsed_ms(e0, e1, which == 0 ? &ms_sym : &ms_csr) == 0;
      }
      if (e0) cfs_hip_event_destroy(e0);
      if (e1) cfs_hip_event_destroy(e1);
      if (xd) cfs_hip_free(xd, CFS_HIP_MEM_DEVICE);
      if (yd) cfs_hip_free(yd, CFS_HIP_MEM_DEVICE);
      if (ok && ms_csr < 0.9f * ms_sym) { // the general kernel wins clearly: keep it
        std::cout << "[INFO]: symmetric tile schedule " << ms_sym / 5 * 1e3 << " us per SpMV, general CSR kernel "
                  << ms_csr / 5 * 1e3 << " us: no locality to exploit -- using the general CSR kernel" << std::endl;
        cfs_hip_sym_destroy((cfs_hip_sym_t)sym_handle_);
        sym_handle_ = nullptr;
        csr_handle_ = g;
        device_bytes_ = ((size_t)nrows_ + 1) * sizeof(IndexT) + (size_t)nnz_ * (sizeof(IndexT) + sizeof(ValueT));
        tuned_ = true;
        return true;
      }
      if (g) cfs_hip_csr_destroy(g);
    }
  }
  if (use_sss) {
    cfs_hip_sym_stats st;
    cfs_hip_sym_get_stats((cfs_hip_sym_t)sym_handle_, &st);
    device_bytes_ = (size_t)st.device_bytes;
#ifdef _LOG_INFO
    std::cout << "[INFO]: " << st.ntiles << " tiles, " << st.halo_slots << " halo slots, "
              << st.far_entries << " far entries, " << st.lds_bytes << " B LDS per workgroup, "
              << cfs::util::runtime::get_num_gpus() << " shard(s)" << std::endl;
#endif
    if (!plan_path.empty() && cfs_hip_sym_save((cfs_hip_sym_t)sym_handle_, plan_path.c_str(), plan_tag.c_str()) != 0)
      std::cout << "[INFO]: plan cache not written: " << cfs_hip_last_error() << std::endl; // best effort
    release_host_csr(); // csr_matrix.tpp:1700-1706
  } else {
    cfs_hip_csr_t h = nullptr;
    if (std::is_same<ValueT, double>::value)
      rc = cfs_hip_csr_create_f64(nrows_, ncols_, rowptr_, colind_, (const double *)values_, &h);
    else
      rc = cfs_hip_csr_create_f32(nrows_, ncols_, rowptr_, colind_, (const float *)values_, &h);
    if (rc != 0) fatal(std::string("tune() failed: ") + cfs_hip_last_error());
    csr_handle_ = h;
    device_bytes_ = ((size_t)nrows_ + 1) * sizeof(IndexT) +
                    (size_t)nnz_ * (sizeof(IndexT) + sizeof(ValueT));
  }
  tuned_ = true;
  return true;
}

template <typename IndexT, typename ValueT>
void CSRMatrix<IndexT, ValueT>::dense_vector_multiply(ValueT *__restrict y,
                                                      const ValueT *__restrict x) {
  int rc;
  if (sym_handle_) rc = cfs_hip_sym_spmv((cfs_hip_sym_t)sym_handle_, y, x);
  else if (csr_handle_) rc = cfs_hip_csr_spmv((cfs_hip_csr_t)csr_handle_, y, x);
  else {
    fatal("dense_vector_multiply() before tune()"); // std::bad_function_call in the reference
    return;
  }
  if (rc != 0) fatal(std::string("SpMV failed: ") + cfs_hip_last_error());
}

template class CSRMatrix<int, float>;
template class CSRMatrix<int, double>;

} // namespace sparse
} // namespace matrix
} // namespace cfs
