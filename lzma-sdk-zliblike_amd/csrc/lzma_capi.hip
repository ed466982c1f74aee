// lzma_capi.hip -- host side of liblzmagpu.so: the batch extension
// (include/lzma_gpu.h: planner, batch launches, streaming sessions, LZMA2
// block splitter) and the library's shared host state
// (device check, per-device call scratch and class-stream pools).  The
// LzmaDec / LzmaLib / Lzma2Dec drop-ins are in dropin_capi.hip.
//
// Without a HIP device every decode entry returns SZ_ERROR_FAIL (no CPU
// fallback).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "host_batch.h"
#include "lzma_device.h"
#include "lzma_gpu_internal.h"

namespace {

thread_local std::string g_last_error;

void set_error(const std::string& s) { g_last_error = s; }

bool hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return false;
}

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// set once the library has started the HIP runtime with a device present
std::atomic<bool> g_runtime_up{false};

bool ensure_device() {
  static std::once_flag once;
  static int count = 0;
  std::call_once(once, [] {
    count = device_count();
    if (count > 0) g_runtime_up.store(true);
  });
  if (count <= 0) {
    set_error("liblzmagpu: no HIP device available (GPU decoder only, no CPU fallback)");
    static std::atomic<bool> warned{false};
    if (!warned.exchange(true))
      fprintf(stderr, "liblzmagpu: no HIP device available -- decode calls return SZ_ERROR_FAIL\n");
    return false;
  }
  return true;
}

// CUs the planner and launchers size for: the current device's, cached per
// device, once ensure_device() has started the runtime; before that (a
// launcher process that plans before it starts its ranks) MI355X's 256, with
// no HIP call -- planning alone never initialises the GPU.
uint32_t device_cus() {
  if (!g_runtime_up.load()) return 256;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kLzgpuMaxDevices) return 256;
  static std::atomic<uint32_t> cache[kLzgpuMaxDevices];
  uint32_t c = cache[dev].load();
  if (c) return c;
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
    return 256;
  cache[dev].store(uint32_t(v));
  return uint32_t(v);
}

int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : dflt;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ batch extension

// The planner is decode_plan.h (plan_simple, plan_batch); its entry points:
size_t LzmaGpu_PlanBatch(LzmaGpuStreamDesc* descs, size_t n, uint32_t* order) {
  try {
    return lzgpu_host::plan_simple(descs, n, order);
  } catch (const std::exception&) {
    set_error("plan: host allocation failed");
    return 0;
  }
}

// Planner defaults with the experiment overrides of the environment, read at
// call time (LZGPU_KERNEL=global|throughput|latency|coop, LZGPU_MASK=1|2,
// LZGPU_COOP=0|1, LZGPU_CUS, LZGPU_LANES, LZGPU_GROUPS, LZGPU_OCC,
// LZGPU_PERSIST=0, LZGPU_CLASSES=1, LZGPU_SLICE_ALIGN8=1, LZGPU_KERNEL_LZMA2=1,
// LZGPU_COOP_LAT=1, LZGPU_MERGE_LAT=0, LZGPU_ILV=0, LZGPU_ILV_ANY=1, LZGPU_THR_FIT=0,
// LZGPU_SLOTG=0).  Only LzmaGpu_PlanBatchEx reads them;
// LzmaGpu_PlanBatchOpt takes its options from the caller alone.
static LzmaGpuPlanOptions env_options() {
  LzmaGpuPlanOptions o;
  memset(&o, 0, sizeof o);
  const char* kv = getenv("LZGPU_KERNEL");
  if (env_int("LZGPU_KERNEL_GLOBAL", 0) || (kv && strcmp(kv, "global") == 0))
    o.kernel = LZMA_GPU_KERNEL_GLOBAL;
  else if (kv && strcmp(kv, "throughput") == 0)
    o.kernel = LZMA_GPU_KERNEL_THROUGHPUT;
  else if (kv && strcmp(kv, "latency") == 0)
    o.kernel = LZMA_GPU_KERNEL_LATENCY;
  else if (kv && strcmp(kv, "coop") == 0)
    o.kernel = LZMA_GPU_KERNEL_COOP;
  const int mask = env_int("LZGPU_MASK", 0), coop = env_int("LZGPU_COOP", -1);
  if (o.kernel == LZMA_GPU_KERNEL_AUTO) {
    if (mask == 1) o.kernel = LZMA_GPU_KERNEL_THROUGHPUT;
    if (mask == 2) o.kernel = coop == 1 ? LZMA_GPU_KERNEL_COOP : LZMA_GPU_KERNEL_LATENCY;
  }
  o.coop = coop < 0 ? 0u : (coop ? 1u : 2u);
  o.cus = uint32_t(std::max(0, env_int("LZGPU_CUS", 0)));
  o.lanes_per_group = uint32_t(std::max(0, env_int("LZGPU_LANES", 0)));
  o.groups_per_cu = uint32_t(std::max(0, env_int("LZGPU_GROUPS", 0)));
  o.waves_per_simd = uint32_t(std::max(0, env_int("LZGPU_OCC", 0)));
  o.persistent = env_int("LZGPU_PERSIST", 1) ? 0u : 2u;
  o.one_class = env_int("LZGPU_CLASSES", 0) == 1 ? 1u : 0u;
  o.flags = (env_int("LZGPU_SLICE_ALIGN8", 0) ? LZMA_GPU_PLAN_SLICE_ALIGN8 : 0u) |
            (env_int("LZGPU_KERNEL_LZMA2", 0) ? LZMA_GPU_PLAN_KERNEL_LZMA2 : 0u) |
            (env_int("LZGPU_COOP_LAT", 0) ? LZMA_GPU_PLAN_COOP_LAT : 0u) |
            (env_int("LZGPU_MERGE_LAT", 1) ? 0u : LZMA_GPU_PLAN_NO_MERGE_LAT) |
            (env_int("LZGPU_ILV", 1) ? 0u : LZMA_GPU_PLAN_NO_ILV) |
            (env_int("LZGPU_ILV_ANY", 0) ? LZMA_GPU_PLAN_ILV_ANY : 0u) |
            (env_int("LZGPU_THR_FIT", 1) ? 0u : LZMA_GPU_PLAN_NO_THR_FIT) |
            (env_int("LZGPU_SLOTG", 1) ? 0u : LZMA_GPU_PLAN_NO_SLOTG);
  return o;
}

SRes LzmaGpu_PlanBatchEx(LzmaGpuStreamDesc* descs, size_t n, uint32_t* order, LzmaGpuPlan* plan) {
  return LzmaGpu_PlanBatchOpt(descs, n, order, plan, nullptr);
}

// C ABI: no exception crosses it (host allocation failure -> SZ_ERROR_MEM).
SRes LzmaGpu_PlanBatchOpt(LzmaGpuStreamDesc* descs, size_t n, uint32_t* order, LzmaGpuPlan* plan,
                          const LzmaGpuPlanOptions* opt) {
  if (opt && (opt->flags & ~LZMA_GPU_PLAN_KNOWN_FLAGS)) return SZ_ERROR_PARAM;
  const LzmaGpuPlanOptions o = opt ? *opt : env_options();
  return lzgpu_host::guarded("plan: host allocation failed", [&]() {
    return lzgpu_host::plan_batch(descs, n, order, plan, o, o.cus ? o.cus : device_cus());
  });
}

// Internal streams for concurrent class launches: a pool per device, guarded
// by a mutex.  A call takes a set for the duration of its enqueueing and puts
// it back; sets are created only when every existing one is taken, so the
// pool grows to the number of threads that enqueue batches at the same time,
// not to the number of threads that ever did.  Reusing a set from another
// thread is safe: work on its streams only orders behind earlier work, and a
// wait on an event captures the event's state at the time of the wait.
struct ClassStreams {
  hipStream_t s[LZMA_GPU_MAX_CLASSES] = {};
  hipEvent_t fork = nullptr, join[LZMA_GPU_MAX_CLASSES] = {};
  int dev = 0;
};
static void destroy_class_streams(ClassStreams* c) {
  if (!c) return;
  for (int k = 0; k < LZMA_GPU_MAX_CLASSES; ++k) {
    if (c->s[k]) (void)hipStreamDestroy(c->s[k]);
    if (c->join[k]) (void)hipEventDestroy(c->join[k]);
  }
  if (c->fork) (void)hipEventDestroy(c->fork);
  delete c;
}
struct ClassStreamPool {
  std::mutex mu;
  std::vector<ClassStreams*> free_sets[kLzgpuMaxDevices];
};
static ClassStreamPool& class_stream_pool() {
  static ClassStreamPool* p = new ClassStreamPool();  // process lifetime (HIP teardown order)
  return *p;
}
static ClassStreams* class_streams_acquire() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kLzgpuMaxDevices) return nullptr;
  ClassStreamPool& P = class_stream_pool();
  {
    std::lock_guard<std::mutex> g(P.mu);
    if (!P.free_sets[dev].empty()) {
      ClassStreams* c = P.free_sets[dev].back();
      P.free_sets[dev].pop_back();
      return c;
    }
  }
  ClassStreams* c = new (std::nothrow) ClassStreams();
  if (!c) return nullptr;
  c->dev = dev;
  bool ok = hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) == hipSuccess;
  for (int k = 0; k < LZMA_GPU_MAX_CLASSES && ok; ++k)
    ok = hipStreamCreateWithFlags(&c->s[k], hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&c->join[k], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    destroy_class_streams(c);  // whatever part of the set was created
    (void)hipGetLastError();
    return nullptr;
  }
  return c;
}
static void class_streams_release(ClassStreams* c) {
  if (!c) return;
  ClassStreamPool& P = class_stream_pool();
  std::lock_guard<std::mutex> g(P.mu);
  try {
    P.free_sets[c->dev].push_back(c);
  } catch (const std::exception&) {
    destroy_class_streams(c);
  }
}

SRes LzmaGpu_DecodeBatchEx(const LzmaGpuPlan* plan, const LzmaGpuStreamDesc* d_descs,
                           const uint32_t* d_order, const Byte* d_src, Byte* d_dst,
                           void* d_workspace, LzmaGpuResult* d_results, void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (!plan || !d_order || plan->n > 0xFFFFFFFFull || plan->n_lds > plan->n ||
      plan->n_classes > LZMA_GPU_MAX_CLASSES)
    return SZ_ERROR_PARAM;
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint16_t* ws = static_cast<uint16_t*>(d_workspace);
  const uint32_t cus = device_cus();
  // Several width classes (mixed lc/lp/pb batches, config 5): each class is a
  // persistent launch whose workgroups leave only when its queue is drained,
  // so on one stream every class ends in a tail of a few long streams while
  // the rest of the chip idles.  On their own streams (forked from and joined
  // back into the caller's) the next class's workgroups fill the CUs the
  // previous one frees.  LZGPU_CLASS_STREAMS=0: one stream (A/B).
  uint32_t live = 0;
  for (uint32_t k = 0; k < plan->n_classes; ++k) live += plan->classes[k].n ? 1u : 0u;
  {
    uint64_t sum = 0;
    for (uint32_t k = 0; k < plan->n_classes; ++k) sum += plan->classes[k].n;
    if (sum > plan->n_lds) return SZ_ERROR_PARAM;
  }
  const bool fork = live > 1 && env_int("LZGPU_CLASS_STREAMS", 1) != 0;
  // concurrent classes are a speed-up only: without a stream set (resource
  // exhaustion) the classes run one after another on the caller's stream
  ClassStreams* cs = fork ? class_streams_acquire() : nullptr;
  if (cs && hipEventRecord(cs->fork, st) != hipSuccess) {
    (void)hipGetLastError();
    class_streams_release(cs);
    cs = nullptr;
  }
  SRes ret = SZ_OK;
  uint64_t first = 0;
  for (uint32_t k = 0; k < plan->n_classes && ret == SZ_OK; ++k) {
    const LzmaGpuLdsClass& c = plan->classes[k];
    if (c.n == 0) continue;
    const uint32_t max_groups = plan->persistent ? cus * c.groups_per_cu : 0u;
    uint32_t* queue = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(d_workspace) +
                                                  plan->queue_offset + 64 * k);
    hipStream_t sk = st;
    if (cs) {
      sk = cs->s[k];
      if (!hip_ok(hipStreamWaitEvent(sk, cs->fork, 0), "class fork")) {
        ret = SZ_ERROR_FAIL;
        break;
      }
    }
    const LzgpuDecodeBufs bufs{d_descs, d_order + first, d_src, d_dst, ws, d_results, queue};
    if (lzgpu_launch_decode_lds(c, bufs, max_groups, sk) != 0) {
      set_error("LDS decode kernel launch failed");
      ret = SZ_ERROR_FAIL;
      break;
    }
    if (cs && (!hip_ok(hipEventRecord(cs->join[k], sk), "class join") ||
               !hip_ok(hipStreamWaitEvent(st, cs->join[k], 0), "class join"))) {
      ret = SZ_ERROR_FAIL;
      break;
    }
    first += c.n;
  }
  class_streams_release(cs);
  if (ret != SZ_OK) return ret;
  const uint32_t n_lds = uint32_t(plan->n_lds), n_glob = uint32_t(plan->n - plan->n_lds);
  if (n_glob && lzgpu_launch_decode_batch(d_descs, d_order + n_lds, n_glob, d_src, d_dst, ws,
                                          d_results, st) != 0) {
    set_error("generic decode kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  return SZ_OK;
}

SRes LzmaGpu_DecodeBatch(const LzmaGpuStreamDesc* d_descs, const uint32_t* d_order, size_t n,
                         const Byte* d_src, Byte* d_dst, void* d_workspace, size_t workspace_bytes,
                         LzmaGpuResult* d_results, void* stream) {
  (void)workspace_bytes;
  return lzgpu_host::batch_launch("batch", n, [&]() {
    return lzgpu_launch_decode_batch(d_descs, d_order, uint32_t(n), d_src, d_dst,
                                     static_cast<uint16_t*>(d_workspace), d_results,
                                     static_cast<hipStream_t>(stream));
  });
}

static SRes decode_batch_host(const LzmaGpuStreamDesc* descs, size_t n, const Byte* src,
                              size_t src_bytes, Byte* dst, size_t dst_bytes,
                              LzmaGpuResult* results, const LzmaGpuPlanOptions* opt,
                              LzmaGpuPlan* plan_out) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n == 0) return SZ_OK;
  std::vector<LzmaGpuStreamDesc> d(descs, descs + n);
  std::vector<uint32_t> order(n);
  LzmaGpuPlan plan;
  {
    const SRes pr = LzmaGpu_PlanBatchOpt(d.data(), n, order.data(), &plan, opt);
    if (pr != SZ_OK) return pr;
  }
  if (plan_out) *plan_out = plan;
  lzgpu_host::DevArr<Byte> d_src, d_dst, d_ws;
  lzgpu_host::DevArr<LzmaGpuStreamDesc> d_desc;
  lzgpu_host::DevArr<uint32_t> d_order;
  lzgpu_host::DevArr<LzmaGpuResult> d_res;
  SRes r = lzgpu_host::alloc_all("batch", d_src, src_bytes, d_dst, dst_bytes, d_ws,
                                 size_t(plan.workspace_bytes), d_res, n);
  if (r != SZ_OK) return r;
  if (src_bytes && !hip_ok(hipMemcpy(d_src.p, src, src_bytes, hipMemcpyHostToDevice), "H2D src"))
    return SZ_ERROR_FAIL;
  if ((r = lzgpu_host::upload(d_desc, d, "batch")) != SZ_OK ||
      (r = lzgpu_host::upload(d_order, order, "batch")) != SZ_OK)
    return r;
  if (LzmaGpu_DecodeBatchEx(&plan, d_desc.p, d_order.p, d_src.p, d_dst.p, d_ws.p, d_res.p,
                            nullptr) != SZ_OK ||
      !hip_ok(hipDeviceSynchronize(), "decode kernel") ||
      !hip_ok(hipMemcpy(results, d_res.p, n * sizeof(LzmaGpuResult), hipMemcpyDeviceToHost),
              "D2H results") ||
      (dst_bytes && !hip_ok(hipMemcpy(dst, d_dst.p, dst_bytes, hipMemcpyDeviceToHost), "D2H dst")))
    return SZ_ERROR_FAIL;
  return SZ_OK;
}

SRes LzmaGpu_DecodeBatchHostOpt(const LzmaGpuStreamDesc* descs, size_t n, const Byte* src,
                                size_t src_bytes, Byte* dst, size_t dst_bytes,
                                LzmaGpuResult* results, const LzmaGpuPlanOptions* opt,
                                LzmaGpuPlan* plan_out) {
  return lzgpu_host::guarded("batch: host allocation failed", [&]() {
    return decode_batch_host(descs, n, src, src_bytes, dst, dst_bytes, results, opt, plan_out);
  });
}

SRes LzmaGpu_DecodeBatchHost(const LzmaGpuStreamDesc* descs, size_t n, const Byte* src,
                             size_t src_bytes, Byte* dst, size_t dst_bytes,
                             LzmaGpuResult* results) {
  return LzmaGpu_DecodeBatchHostOpt(descs, n, src, src_bytes, dst, dst_bytes, results, nullptr,
                                    nullptr);
}

size_t Lzma2Gpu_SplitBlocks(const Byte* src, size_t src_len, uint64_t* src_off,
                            uint64_t* block_src_len, uint64_t* unpack, size_t max_blocks) {
  size_t pos = 0, nb = 0;
  uint64_t cur_unpack = 0;
  bool open = false;
  auto close_block = [&](size_t end) {
    if (open && nb - 1 < max_blocks) {
      block_src_len[nb - 1] = end - src_off[nb - 1];
      unpack[nb - 1] = cur_unpack;
    }
  };
  while (pos < src_len) {
    const Byte c = src[pos];
    if (c == 0) {
      close_block(pos);
      return nb;
    }
    const bool is_lzma = (c & 0x80) != 0;
    if (!is_lzma && c > 2) return size_t(-1);
    const bool reset = (c == 1) || (c >= 0xE0);
    if (reset) {
      close_block(pos);
      if (nb < max_blocks) src_off[nb] = pos;
      nb++;
      open = true;
      cur_unpack = 0;
    } else if (!open) {
      return size_t(-1);  // stream must start with a dictionary reset
    }
    if (is_lzma) {
      if (pos + 5 > src_len) return size_t(-1);
      const uint64_t u = (uint64_t(c & 0x1F) << 16) + (uint64_t(src[pos + 1]) << 8) + src[pos + 2] + 1;
      const uint64_t pk = (uint64_t(src[pos + 3]) << 8) + src[pos + 4] + 1;
      const size_t hdr = (((c >> 5) & 3) >= 2) ? 6 : 5;
      cur_unpack += u;
      pos += hdr + pk;
    } else {
      if (pos + 3 > src_len) return size_t(-1);
      const uint64_t u = (uint64_t(src[pos + 1]) << 8) + src[pos + 2] + 1;
      cur_unpack += u;
      pos += 3 + u;
    }
  }
  if (pos > src_len) return size_t(-1);
  close_block(src_len);  // no EOS byte: the last block runs to the end
  return nb;
}

// ------------------------------------------------------------------ streaming sessions

static_assert(sizeof(LzmaGpuSession) == 192, "LzmaGpuSession layout");
static_assert(sizeof(LzmaGpuPlan) == 248, "LzmaGpuPlan layout");

size_t LzmaGpu_SessionProbsBytes(const Byte* props, unsigned propsSize) {
  CLzmaProps pr;
  if (LzmaProps_Decode(&pr, props, propsSize) != SZ_OK) return 0;
  return size_t(lzgpu::table_cells(pr.lc, pr.lp, pr.pb)) * 2;
}

SRes LzmaGpu_SessionInit(LzmaGpuSession* s, const Byte* props, unsigned propsSize,
                         uint16_t* d_probs, Byte* d_dic, size_t dic_buf_size) {
  if (!s) return SZ_ERROR_PARAM;
  CLzmaProps pr;
  const SRes r = LzmaProps_Decode(&pr, props, propsSize);
  if (r != SZ_OK) return r;
  if (!d_probs || !d_dic || dic_buf_size == 0) return SZ_ERROR_PARAM;
  memset(s, 0, sizeof *s);
  s->lc = pr.lc;
  s->lp = pr.lp;
  s->pb = pr.pb;
  s->dict_size = pr.dicSize;
  s->probs = d_probs;
  s->dic = d_dic;
  s->dic_buf_size = dic_buf_size;
  // LzmaDec_Init (LzmaDec.c:701-705): dicPos = 0, InitDicAndState(True, True)
  s->dic_pos = 0;
  s->need_flush = 1;
  s->remain_len = 0;
  s->temp_buf_size = 0;
  s->processed_pos = 0;
  s->check_dic_size = 0;
  s->need_init_state = 1;
  return SZ_OK;
}

SRes LzmaGpu_SessionDecodeBatch(LzmaGpuSession* d_sessions, size_t n, void* stream) {
  return lzgpu_host::batch_launch("session", n, [&]() {
    return lzgpu_launch_session(d_sessions, uint32_t(n), static_cast<hipStream_t>(stream));
  });
}

int LzmaGpu_DeviceCount(void) { return device_count(); }

const char* LzmaGpu_LastError(void) { return g_last_error.c_str(); }

const char* LzmaGpu_Version(void) { return "liblzmagpu 0.1 (gfx950, LZMA SDK 9.20 decoder contract)"; }

}  // extern "C"

namespace lzgpu_host {
bool ensure_device() { return ::ensure_device(); }
void set_error(const char* what) { ::set_error(what); }
bool hip_ok(hipError_t e, const char* what) { return ::hip_ok(e, what); }
uint32_t device_cus() { return ::device_cus(); }

namespace {
struct ScratchPool {
  std::mutex mu;
  std::vector<CallScratch*> free_sets[kLzgpuMaxDevices];
};
ScratchPool& scratch_pool() {
  static ScratchPool* p = new ScratchPool();  // process lifetime (HIP teardown order)
  return *p;
}
}  // namespace

CallScratch* scratch_acquire() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kLzgpuMaxDevices) {
    ::set_error("scratch: no current device");
    return nullptr;
  }
  ScratchPool& P = scratch_pool();
  {
    std::lock_guard<std::mutex> g(P.mu);
    if (!P.free_sets[dev].empty()) {
      CallScratch* s = P.free_sets[dev].back();
      P.free_sets[dev].pop_back();
      return s;
    }
  }
  CallScratch* s = new (std::nothrow) CallScratch();
  if (!s) {
    ::set_error("scratch: host allocation failed");
    return nullptr;
  }
  s->dev = dev;
  if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    ::set_error("scratch: stream creation failed");
    delete s;
    return nullptr;
  }
  return s;
}

uint8_t* scratch_pinned(CallScratch* s, size_t n) {
  if (!s || n > kPinnedStageMax) return nullptr;
  if (s->pin_cap >= n) return s->pin;
  const size_t want = std::min(kPinnedStageMax, std::max({n, s->pin_cap * 2, size_t(256) << 10}));
  if (s->pin) (void)hipHostFree(s->pin);
  s->pin = nullptr;
  s->pin_cap = 0;
  if (hipHostMalloc(reinterpret_cast<void**>(&s->pin), want, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    s->pin = nullptr;
    return nullptr;
  }
  s->pin_cap = want;
  return s->pin;
}

void scratch_release(CallScratch* s) {
  if (!s) return;
  ScratchPool& P = scratch_pool();
  std::lock_guard<std::mutex> g(P.mu);
  try {
    P.free_sets[s->dev].push_back(s);
  } catch (const std::exception&) {
    (void)hipStreamDestroy(s->stream);
    if (s->pin) (void)hipHostFree(s->pin);
    delete s;
  }
}
}  // namespace lzgpu_host
