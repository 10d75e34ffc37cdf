// rphedge native runtime: hipGraph capture/replay, RCCL communicator over
// xGMI, layout tables and small device helpers.  Exposed as a C ABI and
// bound from Python with ctypes (rphedge/ops/native.py) — no torch C++ ABI
// dependency, so the library loads into the torch process and shares its HIP
// runtime (same SONAME libamdhip64.so.7) and RCCL (librccl.so.1).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rph_layout.h"

using namespace rph;

static thread_local char g_err[512];

static int set_err(const char* what, int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s failed (%d): %s", what, code, msg ? msg : "");
  return code == 0 ? -1 : code;
}

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) return set_err(#expr, (int)_e, hipGetErrorString(_e));   \
  } while (0)

#define NCCL_TRY(expr)                                                             \
  do {                                                                             \
    ncclResult_t _r = (expr);                                                      \
    if (_r != ncclSuccess) return set_err(#expr, (int)_r, ncclGetErrorString(_r)); \
  } while (0)

extern "C" const char* rph_last_error() { return g_err; }

// descriptor validation failures from the kernel launchers (hedge_mlp.hip)
namespace rph {
int rph_report(const char* what, const char* msg) { return set_err(what, -22, msg); }
int rph_report_shape(const char* what, int nin, int h, int nout, int head) {
  char msg[128];
  snprintf(msg, sizeof(msg), "unsupported network shape (nin %d, h %d, nout %d, head %d)", nin, h, nout, head);
  return rph_report(what, msg);
}
}  // namespace rph

// ---------------------------------------------------------------------------
// Layout tables (rph_layout.h): the Python mirrors are compared with them by
// name when the library is loaded.
// ---------------------------------------------------------------------------
extern "C" int rph_layout_fields(const FieldRow** rows) {
  *rows = kFieldRows;
  return (int)(sizeof(kFieldRows) / sizeof(kFieldRows[0]));
}

extern "C" int rph_layout_fields_ext(const FieldRow** rows) {
  *rows = kFieldRowsExt;
  return (int)(sizeof(kFieldRowsExt) / sizeof(kFieldRowsExt[0]));
}

extern "C" int rph_layout_fields_ride(const FieldRow** rows) {
  *rows = kFieldRowsRide;
  return (int)(sizeof(kFieldRowsRide) / sizeof(kFieldRowsRide[0]));
}

extern "C" int rph_layout_fields_sim(const FieldRow** rows) {
  *rows = kFieldRowsSim;
  return (int)(sizeof(kFieldRowsSim) / sizeof(kFieldRowsSim[0]));
}

extern "C" int rph_layout_fields_cost(const FieldRow** rows) {
  *rows = kFieldRowsCost;
  return (int)(sizeof(kFieldRowsCost) / sizeof(kFieldRowsCost[0]));
}

extern "C" int rph_layout_fields_jump(const FieldRow** rows) {
  *rows = kFieldRowsJump;
  return (int)(sizeof(kFieldRowsJump) / sizeof(kFieldRowsJump[0]));
}

extern "C" int rph_layout_consts_cost(const ConstRow** rows) {
  *rows = kConstRowsCost;
  return (int)(sizeof(kConstRowsCost) / sizeof(kConstRowsCost[0]));
}

extern "C" int rph_layout_consts(const ConstRow** rows) {
  *rows = kConstRows;
  return (int)(sizeof(kConstRows) / sizeof(kConstRows[0]));
}

// ---------------------------------------------------------------------------
// Device helpers
// ---------------------------------------------------------------------------
extern "C" int rph_device_info(int dev, int* cus, int* lds_per_cu, long long* hbm_bytes, char* name, int name_cap) {
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, dev));
  *cus = p.multiProcessorCount;
  *lds_per_cu = (int)p.maxSharedMemoryPerMultiProcessor;
  *hbm_bytes = (long long)p.totalGlobalMem;
  snprintf(name, name_cap, "%s", p.gcnArchName);
  return 0;
}

extern "C" int rph_memset_async(void* ptr, int value, long long bytes, void* stream) {
  HIP_TRY(hipMemsetAsync(ptr, value, (size_t)bytes, (hipStream_t)stream));
  return 0;
}

extern "C" int rph_stream_sync(void* stream) {
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

// ---------------------------------------------------------------------------
// hipGraph capture / replay of whole training scans.
// ---------------------------------------------------------------------------
extern "C" int rph_graph_begin(void* stream) {
  HIP_TRY(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
  return 0;
}

extern "C" int rph_graph_end(void* stream, void** exec_out, long long* num_nodes) {
  hipGraph_t g = nullptr;
  HIP_TRY(hipStreamEndCapture((hipStream_t)stream, &g));
  size_t nn = 0;
  HIP_TRY(hipGraphGetNodes(g, nullptr, &nn));
  *num_nodes = (long long)nn;
  hipGraphExec_t ex = nullptr;
  HIP_TRY(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
  HIP_TRY(hipGraphDestroy(g));
  *exec_out = (void*)ex;
  return 0;
}

extern "C" int rph_graph_launch(void* exec, void* stream) {
  HIP_TRY(hipGraphLaunch((hipGraphExec_t)exec, (hipStream_t)stream));
  return 0;
}

extern "C" int rph_graph_destroy(void* exec) {
  HIP_TRY(hipGraphExecDestroy((hipGraphExec_t)exec));
  return 0;
}

// ---------------------------------------------------------------------------
// RCCL communicator (one per process/GPU).  The 128-byte unique id is
// generated on rank 0 and broadcast through the torch.distributed store by the
// Python side.  All-reduces are enqueued on the caller's (compute) stream so
// they can be captured into the same hipGraph as the training steps.
// ---------------------------------------------------------------------------
extern "C" int rph_nccl_unique_id(char* out128) {
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  memcpy(out128, &id, sizeof(id));
  return (int)sizeof(id);
}

extern "C" int rph_nccl_init(const char* id128, int nranks, int rank, void** comm_out) {
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  ncclComm_t c = nullptr;
  NCCL_TRY(ncclCommInitRank(&c, nranks, id, rank));
  *comm_out = (void*)c;
  return 0;
}

extern "C" int rph_nccl_allreduce_f32(void* comm, void* buf, long long count, void* stream) {
  NCCL_TRY(ncclAllReduce(buf, buf, (size_t)count, ncclFloat32, ncclSum, (ncclComm_t)comm, (hipStream_t)stream));
  return 0;
}

extern "C" int rph_nccl_allreduce_f64(void* comm, void* buf, long long count, void* stream) {
  NCCL_TRY(ncclAllReduce(buf, buf, (size_t)count, ncclFloat64, ncclSum, (ncclComm_t)comm, (hipStream_t)stream));
  return 0;
}

extern "C" int rph_nccl_allreduce_u32(void* comm, void* buf, long long count, void* stream) {
  NCCL_TRY(ncclAllReduce(buf, buf, (size_t)count, ncclUint32, ncclSum, (ncclComm_t)comm, (hipStream_t)stream));
  return 0;
}

extern "C" int rph_nccl_destroy(void* comm) {
  NCCL_TRY(ncclCommDestroy((ncclComm_t)comm));
  return 0;
}

// ---------------------------------------------------------------------------
// IPC mailboxes for the fused xGMI all-reduce (one allocation per rank,
// exported with hipIpcGetMemHandle and opened by every peer process).
// ---------------------------------------------------------------------------
// Mailboxes are written by PEER GPUs over xGMI and polled locally, so they are
// allocated fine-grained (coherent across devices by memory type) when the
// driver can export such an allocation; otherwise coarse-grained hipMalloc
// (the kernels use system-scope stores/loads either way).
static int g_ipc_finegrained = -1;  // 1/0 once decided

extern "C" int rph_ipc_alloc(long long bytes, void** ptr_out, char* handle_out /*64 B*/) {
  void* p = nullptr;
  hipIpcMemHandle_t h;
  bool done = false;
  if (g_ipc_finegrained != 0 && hipExtMallocWithFlags(&p, (size_t)bytes, hipDeviceMallocFinegrained) == hipSuccess) {
    if (hipIpcGetMemHandle(&h, p) == hipSuccess) {
      done = true;
      g_ipc_finegrained = 1;
    } else {
      (void)hipGetLastError();
      (void)hipFree(p);
      p = nullptr;
      g_ipc_finegrained = 0;
    }
  } else {
    (void)hipGetLastError();
  }
  if (!done) {
    HIP_TRY(hipMalloc(&p, (size_t)bytes));
    HIP_TRY(hipIpcGetMemHandle(&h, p));
  }
  HIP_TRY(hipMemset(p, 0, (size_t)bytes));
  HIP_TRY(hipDeviceSynchronize());
  memcpy(handle_out, &h, sizeof(h));
  *ptr_out = p;
  return 0;
}

extern "C" int rph_ipc_is_finegrained() { return g_ipc_finegrained; }

extern "C" int rph_ipc_open(const char* handle /*64 B*/, void** ptr_out) {
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof(h));
  void* p = nullptr;
  HIP_TRY(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
  *ptr_out = p;
  return 0;
}

extern "C" int rph_ipc_close(void* p) {
  HIP_TRY(hipIpcCloseMemHandle(p));
  return 0;
}

extern "C" int rph_free(void* p) {
  HIP_TRY(hipFree(p));
  return 0;
}

extern "C" int rph_ipc_handle_size() { return (int)sizeof(hipIpcMemHandle_t); }
