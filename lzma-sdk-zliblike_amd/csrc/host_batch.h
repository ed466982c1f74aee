// host_batch.h -- the host-buffer plumbing the C-ABI translation units share:
// device arrays and copies with one failure path, the exception guard of an
// entry point, the batch driver that runs a launch_plan.h layout, check values
// and branch filters over host-known ranges of a device buffer.  Header-only:
// a translation unit links only against what it instantiates.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <exception>
#include <string>
#include <vector>

#include "../../include/lzma_gpu.h"
#include "launch_plan.h"
#include "lzma_gpu_internal.h"

namespace lzgpu_host {

// The body of a C-ABI entry point: no exception crosses the ABI, a failed host
// allocation is SZ_ERROR_MEM with `what` as the error text.
template <class F>
SRes guarded(const char* what, F f) {
  try {
    return f();
  } catch (const std::exception&) {
    set_error(what);
    return SZ_ERROR_MEM;
  }
}

// The body of a device-pointer entry point that is one launch over n items
// (launch() returns 0 on success): no device is SZ_ERROR_FAIL, a count the
// kernels' 32-bit indices cannot hold is SZ_ERROR_PARAM, a failed launch is
// "<what> kernel launch failed" and SZ_ERROR_FAIL.
template <class Launch>
SRes batch_launch(const char* what, size_t n, Launch launch) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0xFFFFFFFFull) return SZ_ERROR_PARAM;
  if (launch() != 0) {
    set_error((std::string(what) + " kernel launch failed").c_str());
    return SZ_ERROR_FAIL;
  }
  return SZ_OK;
}

// ---------------------------------------------------------------- arrays and copies

inline bool alloc_each() { return true; }
template <class T, class... Rest>
bool alloc_each(DevArr<T>& a, size_t n, Rest&&... rest) {
  return a.alloc(n) && alloc_each(rest...);
}
// alloc_all(what, array, count, array, count, ...): the one failure path of a
// device allocation -- HIP's last error is cleared (the process's next launch
// check must not see it), "<what>: device allocation failed", SZ_ERROR_MEM.
template <class... A>
SRes alloc_all(const char* what, A&&... arrays) {
  if (alloc_each(arrays...)) return SZ_OK;
  (void)hipGetLastError();
  set_error((std::string(what) + ": device allocation failed").c_str());
  return SZ_ERROR_MEM;
}

template <class T>
SRes upload(DevArr<T>& g, const std::vector<T>& h, const char* what) {
  const SRes r = alloc_all(what, g, h.size());
  if (r != SZ_OK) return r;
  return h.empty() || hip_ok(hipMemcpy(g.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice),
                             what)
             ? SZ_OK
             : SZ_ERROR_FAIL;
}
// h.size() elements from d
template <class T>
bool download(std::vector<T>& h, const T* d, const char* what) {
  return h.empty() ||
         hip_ok(hipMemcpy(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost), what);
}

// a workspace limit of 0 is the library's choice: half of the free device memory
inline bool default_workspace_limit(uint64_t& limit) {
  if (limit != 0) return true;
  size_t free_b = 0, total_b = 0;
  if (!hip_ok(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo")) return false;
  limit = free_b / 2;
  return true;
}

// ---------------------------------------------------------------- the batch driver

// The descriptors as the device sees them, each with its workspace offset: in
// launch order (a launch is a contiguous run of them, its results are scattered
// back through p.order), or in caller order (the kernel walks a device copy of
// p.order and writes results at the caller's index).
template <class Desc>
std::vector<Desc> in_launch_order(const Desc* descs, const LaunchPlan& p) {
  std::vector<Desc> d(p.order.size());
  for (size_t k = 0; k < d.size(); ++k) {
    d[k] = descs[p.order[k]];
    d[k].ws_off = p.ws_off[k];
  }
  return d;
}
template <class Desc>
std::vector<Desc> in_caller_order(const Desc* descs, const LaunchPlan& p) {
  std::vector<Desc> d(descs, descs + p.order.size());
  for (size_t k = 0; k < d.size(); ++k) d[p.order[k]].ws_off = p.ws_off[k];
  return d;
}

// for descriptors that carry no workspace offset (the kernels lay a launch's
// scratch out themselves): launch order only
template <class Desc>
std::vector<Desc> in_plan_order(const Desc* descs, const LaunchPlan& p) {
  std::vector<Desc> d(p.order.size());
  for (size_t k = 0; k < d.size(); ++k) d[k] = descs[p.order[k]];
  return d;
}

// launch(lo, cnt) once per cut of the plan; it picks its own pointers and
// returns 0 on success
template <class Launch>
SRes queue_launches(const char* what, const LaunchPlan& p, Launch launch) {
  for (size_t c = 0; c + 1 < p.cut.size(); ++c) {
    const size_t lo = p.cut[c], cnt = p.cut[c + 1] - lo;
    if (cnt == 0) continue;
    if (launch(uint32_t(lo), uint32_t(cnt)) != 0) {
      set_error((std::string(what) + " kernel launch failed").c_str());
      return SZ_ERROR_FAIL;
    }
  }
  return SZ_OK;
}

// The device side of one host batch call.  The arrays are the caller's to use
// between queue() and the end of the call (compaction, partial downloads).
template <class Desc, class Res>
struct HostBatch {
  LaunchPlan plan;
  DevArr<uint8_t> src, dst, ws;
  DevArr<Desc> desc;
  DevArr<Res> res;
  DevArr<uint32_t> order;  // only with descriptors in caller order
  uint64_t ws_fixed = 0;   // workspace bytes of a launch beside its streams' slices

  // What is checked before anything is allocated: every range lies in its
  // buffer (dst_bytes(d): the stream's range in dst), and the layout of the
  // streams -- work(d) is what a stream's run time grows with, slice(d) its
  // workspace bytes -- under the limit (0: default_workspace_limit).
  template <class DstBytes, class Work, class Slice>
  SRes lay_out(const char* what, const Desc* descs, size_t n, size_t src_size, size_t dst_size,
               uint64_t limit, DstBytes dst_bytes, Work work, Slice slice) {
    return lay_out_ranges(
        what, descs, n, limit,
        [&](const Desc& d) {
          return d.src_off <= src_size && d.src_len <= src_size - d.src_off &&
                 d.dst_off <= dst_size && dst_bytes(d) <= dst_size - d.dst_off;
        },
        work, slice);
  }
  // lay_out with the caller's own range check (in_range(d): every range of the
  // stream lies in its buffer)
  template <class InRange, class Work, class Slice>
  SRes lay_out_ranges(const char* what, const Desc* descs, size_t n, uint64_t limit,
                      InRange in_range, Work work, Slice slice) {
    if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
    for (size_t i = 0; i < n; ++i)
      if (!in_range(descs[i])) return SZ_ERROR_PARAM;
    if (!default_workspace_limit(limit)) return SZ_ERROR_FAIL;
    // the launches' slices share the limit with the fixed part
    if (!launch_plan(n, [&](uint32_t i) { return work(descs[i]); },
                     [&](uint32_t i) { return slice(descs[i]); },
                     limit > ws_fixed ? limit - ws_fixed : 0, plan)) {
      set_error((std::string(what) + ": one stream's workspace slice exceeds the limit").c_str());
      return SZ_ERROR_MEM;
    }
    return SZ_OK;
  }

  // Allocates the arrays, uploads src, dst (dst_init null: left as allocated),
  // the descriptors `d` (in_launch_order or in_caller_order of the plan) and,
  // with_order, the plan's order, then queues the plan's launches on the null
  // stream.  The caller waits.
  template <class Launch>
  SRes queue(const char* what, const std::vector<Desc>& d, bool with_order, const Byte* src_host,
             size_t src_size, const Byte* dst_init, size_t dst_size, Launch launch) {
    const size_t n = d.size();
    SRes r =
        alloc_all(what, src, src_size, dst, dst_size, ws, size_t(plan.ws_max + ws_fixed), desc, n,
                  res, n);
    if (r == SZ_OK && with_order) r = alloc_all(what, order, n);
    if (r != SZ_OK) return r;
    if (!hip_ok(hipMemcpy(src.p, src_host, src_size, hipMemcpyHostToDevice), "upload src") ||
        (dst_init &&
         !hip_ok(hipMemcpy(dst.p, dst_init, dst_size, hipMemcpyHostToDevice), "upload dst")) ||
        !hip_ok(hipMemcpy(desc.p, d.data(), n * sizeof(Desc), hipMemcpyHostToDevice),
                "upload descs") ||
        (with_order && !hip_ok(hipMemcpy(order.p, plan.order.data(), n * sizeof(uint32_t),
                                         hipMemcpyHostToDevice), "upload order")))
      return SZ_ERROR_FAIL;
    return queue_launches(what, plan, launch);
  }

  // waits for the device and fetches the n results as the device holds them
  SRes wait(const char* what, Res* r, size_t n) {
    if (!hip_ok(hipDeviceSynchronize(), what) ||
        !hip_ok(hipMemcpy(r, res.p, n * sizeof(Res), hipMemcpyDeviceToHost), "download results"))
      return SZ_ERROR_FAIL;
    return SZ_OK;
  }
  // as wait(), for descriptors in launch order: results[i] is stream i's
  SRes wait_scattered(const char* what, Res* results) {
    std::vector<Res> r(plan.order.size());
    const SRes w = wait(what, r.data(), r.size());
    if (w != SZ_OK) return w;
    for (size_t k = 0; k < r.size(); ++k) results[plan.order[k]] = r[k];
    return SZ_OK;
  }
  bool download_dst(Byte* host, size_t off, size_t len) {
    return len == 0 ||
           hip_ok(hipMemcpy(host + off, dst.p + off, len, hipMemcpyDeviceToHost), "download dst");
  }
};

// ---------------------------------------------------------------- check values of ranges

// CRC-32, CRC-64 or SHA-256 (value_bytes 4, 8 or 32; xz's and 7z's parameters)
// of the ranges [off[i], off[i] + len[i]) of a device buffer: prepare() uploads
// the ranges and the CRC chunk plan, launch() queues the kernels on the null
// stream, fetch() downloads the values once the caller has waited.
struct RangeChecks {
  size_t n = 0, n_chunks = 0;
  unsigned value_bytes = 0;
  DevArr<uint64_t> ranges;  // off | len
  DevArr<uint32_t> plan;    // chunk base | chunk range
  DevArr<uint64_t> chunk;   // the chunks' partial values
  DevArr<uint8_t> value;

  SRes prepare(const char* what, unsigned value_bytes_, const std::vector<uint64_t>& off,
               const std::vector<uint64_t>& len) {
    n = off.size();
    value_bytes = value_bytes_;
    if (n == 0) return SZ_OK;
    std::vector<uint64_t> ol(off);
    ol.insert(ol.end(), len.begin(), len.end());
    SRes r = upload(ranges, ol, what);
    if (r == SZ_OK) r = alloc_all(what, value, n * value_bytes);
    if (r != SZ_OK || value_bytes == 32) return r;
    n_chunks = CrcGpu_PlanChunks(len.data(), n, nullptr, nullptr);
    if (n_chunks == size_t(-1)) return SZ_ERROR_UNSUPPORTED;
    std::vector<uint32_t> cb(n + n_chunks);
    CrcGpu_PlanChunks(len.data(), n, cb.data(), cb.data() + n);
    r = upload(plan, cb, what);
    return r == SZ_OK ? alloc_all(what, chunk, n_chunks) : r;
  }
  SRes launch(const Byte* d_data) {
    if (n == 0) return SZ_OK;
    const uint64_t *off = ranges.p, *len = ranges.p + n;
    if (value_bytes == 32)
      return Sha256Gpu_Batch(d_data, off, len, n, LZMA_GPU_SHA256_AUTO, value.p, nullptr);
    if (value_bytes == 8)
      return Crc64Gpu_Batch(d_data, off, len, n, plan.p, plan.p + n, n_chunks, ~uint64_t(0),
                            ~uint64_t(0), chunk.p, reinterpret_cast<uint64_t*>(value.p), nullptr);
    return CrcGpu_Batch(d_data, off, len, n, plan.p, plan.p + n, n_chunks, 0xFFFFFFFFu,
                        0xFFFFFFFFu, reinterpret_cast<uint32_t*>(chunk.p),
                        reinterpret_cast<uint32_t*>(value.p), nullptr);
  }
  // n * value_bytes bytes, range after range
  bool fetch(void* out, const char* what) {
    return n == 0 ||
           hip_ok(hipMemcpy(out, value.p, n * value_bytes, hipMemcpyDeviceToHost), what);
  }
};

// ---------------------------------------------------------------- filters over ranges

struct FilterJob {
  size_t n = 0;
  DevArr<uint64_t> r64;   // off | len | done
  DevArr<uint32_t> r32;   // ip or distance | x86 state
  DevArr<uint8_t> state;  // delta, 256 bytes per range

  // once the caller has waited: the bytes each range's converter processed
  // (x86 and the BRA family), the x86 states, the first `bytes` delta state bytes
  bool fetch_done(uint64_t* done, const char* what) {
    return hip_ok(hipMemcpy(done, r64.p + 2 * n, 8 * n, hipMemcpyDeviceToHost), what);
  }
  bool fetch_x86_state(uint32_t* st, const char* what) {
    return hip_ok(hipMemcpy(st, r32.p + n, 4 * n, hipMemcpyDeviceToHost), what);
  }
  bool fetch_delta_state(uint8_t* st, size_t bytes, const char* what) {
    return hip_ok(hipMemcpy(st, state.p, bytes, hipMemcpyDeviceToHost), what);
  }
};

// One in-place filter (xz filter ids: 3 delta, 4 x86, 5..9 the BRA family) over
// the ranges [off[i], off[i] + len[i]) of d_data, queued on the null stream;
// prop[i] is range i's start ip or delta distance (null: 0).  The states start
// from x86_state[i] or delta_state[256 i ..], null: 0 (x86_Convert_Init,
// Delta_Init).  j holds the ranges until the caller waits.
inline SRes queue_filter(const char* what, FilterJob& j, uint32_t kind, Byte* d_data,
                         const std::vector<uint64_t>& off, const std::vector<uint64_t>& len,
                         const uint32_t* prop, int encoding, const uint32_t* x86_state = nullptr,
                         const uint8_t* delta_state = nullptr) {
  const size_t n = j.n = off.size();
  if (n == 0) return SZ_OK;
  std::vector<uint64_t> h64(off);
  h64.insert(h64.end(), len.begin(), len.end());
  h64.resize(3 * n, 0);
  std::vector<uint32_t> h32(kind == 4 ? 2 * n : n, 0);
  if (prop) std::copy(prop, prop + n, h32.begin());
  if (kind == 4 && x86_state) std::copy(x86_state, x86_state + n, h32.begin() + n);
  SRes r = upload(j.r64, h64, what);
  if (r == SZ_OK) r = upload(j.r32, h32, what);
  if (r != SZ_OK) return r;
  const uint64_t *d_off = j.r64.p, *d_len = j.r64.p + n;
  if (kind == 3) {
    if ((r = alloc_all(what, j.state, 256 * n)) != SZ_OK) return r;
    if (!hip_ok(delta_state
                    ? hipMemcpy(j.state.p, delta_state, 256 * n, hipMemcpyHostToDevice)
                    : hipMemset(j.state.p, 0, 256 * n),
                what))
      return SZ_ERROR_FAIL;
    return DeltaGpu_Batch(d_data, d_off, d_len, j.r32.p, j.state.p, n, encoding, nullptr);
  }
  if (kind == 4)
    return BcjGpu_X86Batch(d_data, d_off, d_len, j.r32.p, j.r32.p + n, j.r64.p + 2 * n, n, encoding,
                           nullptr);
  return BraGpu_Batch(kind, d_data, d_off, d_len, j.r32.p, j.r64.p + 2 * n, n, encoding, nullptr);
}

}  // namespace lzgpu_host
