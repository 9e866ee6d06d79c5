// ipc_page.hip -- a page of 32-bit words shared by the processes of one host AND by their GPUs' command processors
// (include/rela_amd.h: rela_ipc_page_*): the control plane of the native partition exchange (rela_amd/parallel.py).
//
// The page is pinned host memory that its creator allocates with HIP (hipHostMalloc) and every other process maps through
// the page's IPC handle (hipIpcOpenMemHandle), so a word can be
//   written by a stream   (hipStreamWriteValue32: after everything queued before it, with release semantics),
//   waited for by a stream (hipStreamWaitValue32, >=: a wait of the command processor -- no CU spins, the host goes on),
//   read by a kernel       (the device view of the page), and read, written or waited for by a host thread.
// (The page used to be POSIX shared memory that every process registered with hipHostRegister.  Registering memory a
// process already has is not possible on every platform -- hipHostRegister can fail with hipErrorInvalidValue -- while
// memory HIP allocated itself is pinned wherever HIP runs.)  The creator's host threads read and write the words in place.  A
// mapping of the handle is a device address only: host code of the other processes cannot dereference it, so their host
// threads reach a word through a private stream -- a 4-byte copy to read it, a stream write to store it.  That stream
// is non-blocking and carries nothing else, so such a read waits for no kernel of the process.  The 64-byte handle
// travels in a small POSIX shared-memory object, whose name is what the processes pass around.
// Words used as step counters only grow, so a wait binds to a value and nothing has to be re-armed or acknowledged.
// csrc/ipc_allreduce.hip orders its two phases the same way (and records why interprocess events were given up).
// The reference has no counterpart: its actors, replay and learner share one address space (pyrela/main.py:131-251).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <mutex>

#include "common.h"

using namespace rela_amd;

struct rela_ipc_page {
  int device = 0;
  uint32_t* host = nullptr;  // the creator's view; nullptr in a process that opened the page
  uint32_t* dev = nullptr;
  bool creator = false;
  char name[64] = "";
  // a process that opened the page: its host threads' way to a word
  hipStream_t copy_stream = nullptr;
  uint32_t* staging = nullptr;  // pinned
  std::mutex m;
};

static_assert(sizeof(hipIpcMemHandle_t) == 64, "handle size");

// host threads of a process that opened the page (p->m held)
static hipError_t remote_load(rela_ipc_page* p, int word, uint32_t* value_out) {
  hipError_t e = hipMemcpyAsync(p->staging, p->dev + word, sizeof(uint32_t), hipMemcpyDeviceToHost, p->copy_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->copy_stream);
  if (e == hipSuccess) *value_out = *reinterpret_cast<volatile uint32_t*>(p->staging);
  return e;
}

extern "C" int rela_ipc_page_create(rela_ipc_page** out, char name_out[64], int device) {
  RELA_CHECK(out && name_out, RELA_EINVAL, "rela_ipc_page_create: bad arguments");
  DeviceGuard g(device);
  RELA_CHECK(g.ok, RELA_ENODEV, "rela_ipc_page_create: HIP device %d not available; there is no CPU path", device);
  auto* p = new rela_ipc_page();
  p->device = device, p->creator = true;
  auto fail = [&](int rc) {
    rela_ipc_page_close(p);
    return rc;
  };
  void* m = nullptr;
  void* d = nullptr;
  hipIpcMemHandle_t mh;
  hipError_t e = hipHostMalloc(&m, RELA_IPC_PAGE_BYTES, hipHostMallocMapped);
  if (e == hipSuccess) {
    p->host = reinterpret_cast<uint32_t*>(m);
    memset(p->host, 0, RELA_IPC_PAGE_BYTES);
    e = hipHostGetDevicePointer(&d, p->host, 0);
  }
  if (e == hipSuccess) e = hipIpcGetMemHandle(&mh, p->host);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_last_error("rela_ipc_page_create: a pinned page and its IPC handle: %s", hipGetErrorString(e));
    return fail(RELA_ENODEV);
  }
  p->dev = reinterpret_cast<uint32_t*>(d);
  static std::atomic<int> serial{0};
  timespec t;
  clock_gettime(CLOCK_REALTIME, &t);
  snprintf(p->name, sizeof(p->name), "/rela-amd-page-%d-%d-%lld", (int)getpid(), serial.fetch_add(1), (long long)t.tv_nsec);
  const int fd = shm_open(p->name, O_CREAT | O_EXCL | O_RDWR, 0600);
  const bool written = fd >= 0 && write(fd, &mh, sizeof(mh)) == (ssize_t)sizeof(mh);
  if (fd >= 0) ::close(fd);
  if (!written) {
    if (fd < 0) set_last_error("rela_ipc_page_create: shm_open(%s) failed", p->name);
    else set_last_error("rela_ipc_page_create: writing the page's handle into %s failed", p->name);
    if (fd >= 0) (void)shm_unlink(p->name);
    return fail(RELA_ESTATE);
  }
  memcpy(name_out, p->name, sizeof(p->name));
  *out = p;
  return RELA_OK;
}

extern "C" int rela_ipc_page_open(rela_ipc_page** out, const char* name, int device) {
  RELA_CHECK(out && name && name[0] == '/', RELA_EINVAL, "rela_ipc_page_open: bad arguments");
  DeviceGuard g(device);
  RELA_CHECK(g.ok, RELA_ENODEV, "rela_ipc_page_open: HIP device %d not available; there is no CPU path", device);
  auto* p = new rela_ipc_page();
  p->device = device;
  snprintf(p->name, sizeof(p->name), "%s", name);
  hipIpcMemHandle_t mh;
  const int fd = shm_open(p->name, O_RDWR, 0600);
  const bool got = fd >= 0 && read(fd, &mh, sizeof(mh)) == (ssize_t)sizeof(mh);
  if (fd >= 0) ::close(fd);
  if (!got) {
    if (fd < 0) set_last_error("rela_ipc_page_open: shm_open(%s) failed: another host, or the creator unlinked it already", p->name);
    else set_last_error("rela_ipc_page_open: %s does not hold a page's handle", p->name);
    delete p;
    return RELA_ESTATE;
  }
  void* d = nullptr;
  void* st = nullptr;
  hipError_t e = hipIpcOpenMemHandle(&d, mh, hipIpcMemLazyEnablePeerAccess);
  if (e == hipSuccess) {
    p->dev = reinterpret_cast<uint32_t*>(d);
    e = hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking);
  }
  if (e == hipSuccess) e = hipHostMalloc(&st, sizeof(uint32_t), hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_last_error("rela_ipc_page_open: mapping the page of %s: %s", p->name, hipGetErrorString(e));
    rela_ipc_page_close(p);
    return RELA_ENODEV;
  }
  p->staging = reinterpret_cast<uint32_t*>(st);
  *out = p;
  return RELA_OK;
}

// the creator, once every other process has opened the page: the name goes, the mappings stay
extern "C" int rela_ipc_page_unlink(rela_ipc_page* p) {
  RELA_CHECK(p && p->creator, RELA_EINVAL, "rela_ipc_page_unlink: not the creator");
  (void)shm_unlink(p->name);
  return RELA_OK;
}

extern "C" void rela_ipc_page_close(rela_ipc_page* p) {
  if (!p) return;
  DeviceGuard g(p->device);
  if (p->host || p->dev) (void)hipDeviceSynchronize();  // no stream operation on the page is still queued
  if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
  if (p->staging) (void)hipHostFree(p->staging);
  if (p->creator) {
    if (p->host) (void)hipHostFree(p->host);
  } else if (p->dev) {
    (void)hipIpcCloseMemHandle(p->dev);
  }
  delete p;
}

extern "C" void* rela_ipc_page_host_ptr(rela_ipc_page* p) { return p ? p->host : nullptr; }
extern "C" void* rela_ipc_page_dev_ptr(rela_ipc_page* p) { return p ? p->dev : nullptr; }

#define PAGE_WORD_CHECK(fn) \
  RELA_CHECK(p && word >= 0 && word < RELA_IPC_PAGE_BYTES / 4, RELA_EINVAL, fn ": word %d outside the page", word)

extern "C" int rela_ipc_page_write32(rela_ipc_page* p, int word, uint32_t value, void* stream) {
  PAGE_WORD_CHECK("rela_ipc_page_write32");
  DeviceGuard g(p->device);
  RELA_HIP(hipStreamWriteValue32((hipStream_t)stream, p->dev + word, value, 0));
  return RELA_OK;
}

extern "C" int rela_ipc_page_wait32(rela_ipc_page* p, int word, uint32_t value, void* stream) {
  PAGE_WORD_CHECK("rela_ipc_page_wait32");
  DeviceGuard g(p->device);
  RELA_HIP(hipStreamWaitValue32((hipStream_t)stream, p->dev + word, value, hipStreamWaitValueGte, 0xFFFFFFFFu));
  return RELA_OK;
}

extern "C" int rela_ipc_page_host_store32(rela_ipc_page* p, int word, uint32_t value) {
  PAGE_WORD_CHECK("rela_ipc_page_host_store32");
  if (p->host) {
    reinterpret_cast<std::atomic<uint32_t>*>(p->host + word)->store(value, std::memory_order_release);
    return RELA_OK;
  }
  DeviceGuard g(p->device);
  std::lock_guard<std::mutex> lk(p->m);
  RELA_HIP(hipStreamWriteValue32(p->copy_stream, p->dev + word, value, 0));
  RELA_HIP(hipStreamSynchronize(p->copy_stream));
  return RELA_OK;
}

extern "C" int rela_ipc_page_host_load32(rela_ipc_page* p, int word, uint32_t* value_out) {
  PAGE_WORD_CHECK("rela_ipc_page_host_load32");
  RELA_CHECK(value_out, RELA_EINVAL, "rela_ipc_page_host_load32: bad arguments");
  if (p->host) {
    *value_out = reinterpret_cast<std::atomic<uint32_t>*>(p->host + word)->load(std::memory_order_acquire);
    return RELA_OK;
  }
  DeviceGuard g(p->device);
  std::lock_guard<std::mutex> lk(p->m);
  RELA_HIP(remote_load(p, word, value_out));
  return RELA_OK;
}

// a host thread waits until the word has reached `value` (written by a stream of any process, or by a host thread)
extern "C" int rela_ipc_page_host_wait32(rela_ipc_page* p, int word, uint32_t value, double timeout_s) {
  PAGE_WORD_CHECK("rela_ipc_page_host_wait32");
  timespec t0;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  // the clock is looked at every 256 loads in place, or at every load that is a copy (which takes microseconds itself)
  const uint64_t look = p->host ? 255 : 0;
  for (uint64_t spins = 0;; ++spins) {
    uint32_t now = 0;
    if (int rc = rela_ipc_page_host_load32(p, word, &now)) return rc;
    if ((int32_t)(now - value) >= 0) break;
    if ((spins & look) == look) {
      timespec t1;
      clock_gettime(CLOCK_MONOTONIC, &t1);
      const double dt = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
      RELA_CHECK(dt < timeout_s, RELA_EWOULDBLOCK, "rela_ipc_page_host_wait32: word %d still %u after %.1f s (waiting for %u)", word,
                 now, dt, value);
      if (dt > 0.0005) usleep(20);  // the writer is a learner step away: leave the core to the actor threads
    }
  }
  return RELA_OK;
}

// Do the stream operations work on this page, in this process, on this runtime?  Writes `value` to `word` through a
// private stream, waits for it through the same stream and checks the host's view.  -> 1 / 0 in *ok_out.
extern "C" int rela_ipc_page_selftest(rela_ipc_page* p, int word, uint32_t value, int* ok_out) {
  PAGE_WORD_CHECK("rela_ipc_page_selftest");
  RELA_CHECK(ok_out, RELA_EINVAL, "rela_ipc_page_selftest: bad arguments");
  DeviceGuard g(p->device);
  *ok_out = 0;
  int can = 0;
  hipStream_t st = nullptr;
  if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, p->device) == hipSuccess && can &&
      hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess) {
    uint32_t seen = ~value;
    const bool ok = hipStreamWriteValue32(st, p->dev + word, value, 0) == hipSuccess &&
                    hipStreamWaitValue32(st, p->dev + word, value, hipStreamWaitValueGte, 0xFFFFFFFFu) == hipSuccess &&
                    hipStreamSynchronize(st) == hipSuccess && rela_ipc_page_host_load32(p, word, &seen) == RELA_OK &&
                    seen == value;
    *ok_out = ok ? 1 : 0;
  }
  if (st) (void)hipStreamDestroy(st);
  (void)hipGetLastError();
  return RELA_OK;
}
