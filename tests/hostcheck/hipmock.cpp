// TEST INFRASTRUCTURE. A stand-in for the slice of the HIP runtime that ppde_amd/csrc/ppde_api.hip calls, on host
// memory, so that the HOST side of the C ABI (allocation bookkeeping, copies and their sizes, error paths, stream /
// event / graph object lifetimes) can run under AddressSanitizer + LeakSanitizer in a container without a GPU.
// Kernels are not executed (hipLaunchKernel returns success); "device" memory is calloc'd host memory, so every
// hipMemcpy / hipMemset the host layer issues is bounds-checked by the sanitizer against the matching hipMalloc.
// Every stream, event, graph and executable graph is its own heap object: one the library forgets to destroy
// shows up in the leak report.
// Fault injection: HIPMOCK_FAIL_AT=k makes the k-th fallible call (allocations, stream / event / graph creation)
// return an error, which drives the library's clean-up paths; hipmock_calls() reports how many there were.
// hipmock_launches() / hipmock_allocs() / hipmock_writes() count kernel launches, allocations and copies / fills so far: a call
// that must refuse its arguments "before anything is touched" is checked to move none of them.
// Trace: HIPMOCK_TRACE=FILE appends one line per runtime call to FILE: the call's name, then what identifies it without a pointer
// value -- bytes of an allocation, copy or fill; kernel name (as registered by the host object), grid, block and dynamic LDS of a
// launch; streams and executable graphs as their index in order of
// creation (-1: the null stream). hipmock_note() appends a line of the driver's own
// (walk.h: the message of every refusal). Two builds of the library that issue the same calls leave the same file.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

namespace {
long g_calls = 0, g_fail_at = -1, g_launches = 0, g_allocs = 0, g_writes = 0;
bool g_armed = false;
bool fail_now() {
    if (!g_armed) { const char* e = getenv("HIPMOCK_FAIL_AT"); g_fail_at = e ? atol(e) : -1; g_armed = true; }
    return ++g_calls == g_fail_at;
}
struct Cfg { dim3 grid, block; size_t shmem; hipStream_t stream; };
thread_local Cfg t_cfg;

// (function-local statics: the host object registers its kernels from a static constructor, maybe before this file's own)
std::map<const void*, std::string>& kernel_names() { static auto* m = new std::map<const void*, std::string>; return *m; }
std::map<const void*, long>& stream_index() { static auto* m = new std::map<const void*, long>; return *m; }
std::map<const void*, long>& graph_index() { static auto* m = new std::map<const void*, long>; return *m; }   // executable graphs
long g_streams = 0, g_graphs = 0;
FILE* trace_file() {
    static FILE* f = [] { const char* e = getenv("HIPMOCK_TRACE"); return e && *e ? fopen(e, "a") : (FILE*)nullptr; }();
    return f;
}
long sidx(hipStream_t s) { auto it = stream_index().find((const void*)s); return it == stream_index().end() ? -1 : it->second; }
#define TR(...) do { if (FILE* f_ = trace_file()) { fprintf(f_, __VA_ARGS__); fputc('\n', f_); fflush(f_); } } while (0)
}  // namespace

extern "C" {
long hipmock_calls() { return g_calls; }
long hipmock_launches() { return g_launches; }
long hipmock_allocs() { return g_allocs; }
long hipmock_writes() { return g_writes; }
void hipmock_rearm(long fail_at) { g_calls = 0; g_fail_at = fail_at; g_armed = true; }
void hipmock_note(const char* text) { TR("note %s", text); }

void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* stub, char*, const char* name, unsigned, void*, void*, void*, void*, int*) { kernel_names()[stub] = name; }
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, hipStream_t s) { t_cfg = Cfg{g, b, sh, s}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, hipStream_t* s) { *g = t_cfg.grid; *b = t_cfg.block; *sh = t_cfg.shmem; *s = t_cfg.stream; return hipSuccess; }
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t sh, hipStream_t st) {
    ++g_launches;
    if (trace_file()) {
        auto it = kernel_names().find(f);
        TR("hipLaunchKernel %s grid %u %u %u block %u %u %u lds %zu stream %ld", it == kernel_names().end() ? "?" : it->second.c_str(),
           g.x, g.y, g.z, b.x, b.y, b.z, sh, sidx(st));
    }
    if (g.x == 0 || g.y == 0 || g.z == 0 || b.x == 0 || b.x * b.y * b.z > 1024 || sh > 160 * 1024) return hipErrorInvalidConfiguration;
    return hipSuccess;
}
hipError_t hipExtLaunchKernel(const void* f, dim3 g, dim3 b, void** args, size_t sh, hipStream_t st, hipEvent_t, hipEvent_t stop, int) {
    TR("hipExtLaunchKernel stop_event %d", stop != nullptr);
    return hipLaunchKernel(f, g, b, args, sh, st);
}
hipError_t hipGetDeviceCount(int* n) { TR("hipGetDeviceCount"); *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { TR("hipSetDevice %d", d); return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipGetLastError() { TR("hipGetLastError"); return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory (mock)" : "error (mock)"; }
hipError_t hipDeviceSynchronize() { TR("hipDeviceSynchronize"); return hipSuccess; }

hipError_t hipMalloc(void** p, size_t n) { TR("hipMalloc %zu", n); ++g_allocs; if (fail_now()) { *p = nullptr; return hipErrorOutOfMemory; } *p = calloc(n ? n : 1, 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { TR("hipFree"); free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { TR("hipHostMalloc %zu", n); ++g_allocs; if (fail_now()) { *p = nullptr; return hipErrorOutOfMemory; } *p = calloc(n ? n : 1, 1); return hipSuccess; }
hipError_t hipHostFree(void* p) { TR("hipHostFree"); free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { TR("hipHostGetDevicePointer"); *d = h; return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { TR("hipMemcpy %zu", n); ++g_writes; if (n) memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) { TR("hipMemcpyAsync %zu stream %ld", n, sidx(st)); ++g_writes; if (n) memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemset(void* d, int v, size_t n) { TR("hipMemset %zu", n); ++g_writes; if (n) memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) { TR("hipMemsetAsync %zu stream %ld", n, sidx(st)); ++g_writes; if (n) memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetD32Async(hipDeviceptr_t d, int v, size_t count, hipStream_t st) { TR("hipMemsetD32Async %zu value %d stream %ld", count * 4, v, sidx(st)); ++g_writes; for (size_t i = 0; i < count; ++i) ((int*)d)[i] = v; return hipSuccess; }

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { TR("hipStreamCreateWithFlags"); if (fail_now()) return hipErrorOutOfMemory; *s = (hipStream_t)malloc(8); stream_index()[(const void*)*s] = g_streams++; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { TR("hipStreamDestroy stream %ld", sidx(s)); stream_index().erase((const void*)s); free((void*)s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t st) { TR("hipStreamSynchronize stream %ld", sidx(st)); return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t st) { TR("hipStreamQuery stream %ld", sidx(st)); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t, unsigned) { TR("hipStreamWaitEvent stream %ld", sidx(st)); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { TR("hipEventCreate"); if (fail_now()) return hipErrorOutOfMemory; *e = (hipEvent_t)malloc(8); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { TR("hipEventDestroy"); free((void*)e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t st) { TR("hipEventRecord stream %ld", sidx(st)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { TR("hipEventSynchronize"); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { TR("hipEventElapsedTime"); *ms = 1.0f; return hipSuccess; }
hipError_t hipStreamBeginCapture(hipStream_t st, hipStreamCaptureMode) { TR("hipStreamBeginCapture stream %ld", sidx(st)); return fail_now() ? hipErrorOutOfMemory : hipSuccess; }
hipError_t hipStreamEndCapture(hipStream_t st, hipGraph_t* g) { TR("hipStreamEndCapture stream %ld", sidx(st)); if (fail_now()) { *g = nullptr; return hipErrorOutOfMemory; } *g = (hipGraph_t)malloc(8); return hipSuccess; }
hipError_t hipGraphInstantiate(hipGraphExec_t* x, hipGraph_t, hipGraphNode_t*, char*, size_t) { TR("hipGraphInstantiate"); if (fail_now()) return hipErrorOutOfMemory; *x = (hipGraphExec_t)malloc(8); graph_index()[(const void*)*x] = g_graphs++; return hipSuccess; }
hipError_t hipGraphUpload(hipGraphExec_t x, hipStream_t st) { TR("hipGraphUpload graph %ld stream %ld", graph_index()[(const void*)x], sidx(st)); return hipSuccess; }
hipError_t hipGraphLaunch(hipGraphExec_t x, hipStream_t st) { TR("hipGraphLaunch graph %ld stream %ld", graph_index()[(const void*)x], sidx(st)); return hipSuccess; }
hipError_t hipGraphDestroy(hipGraph_t g) { TR("hipGraphDestroy"); free((void*)g); return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t x) { TR("hipGraphExecDestroy graph %ld", graph_index()[(const void*)x]); graph_index().erase((const void*)x); free((void*)x); return hipSuccess; }
}
