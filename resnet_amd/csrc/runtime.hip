// runtime.hip -- HIP runtime behind mi_device.h (memory, streams, events) and the RCCL binding.
// Replaces the cudaMalloc/cudaMemcpy/cudaDeviceSynchronize calls scattered through resnet.cu
// (e.g. :693-704, :1315-1316, :3342) with stream-ordered equivalents.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <vector>
#include "mi_device.h"
#include "mi_common.hpp"

static char g_err[512] = "";
void mi_record_error(const char *what, const char *detail) {
    if (g_err[0] == 0) snprintf(g_err, sizeof g_err, "%s: %s", what, detail);
}
// ---- launch trace (diagnostic, off unless RESNET_MI_TRACE=1) ----
#include <signal.h>
#include <unistd.h>
#define MI_TRACE_N 96
static const char *g_trace[MI_TRACE_N];
static unsigned g_trace_n = 0;
static int g_trace_on = -1;
static void (*g_trace_prev)(int) = SIG_DFL; /* e.g. Python's faulthandler: runs after the dump */
static void mi_trace_dump(int sig) {
    const char hdr[] = "\nresnet_mi: aborted; last kernel launches, oldest first:\n";
    if (write(2, hdr, sizeof hdr - 1) < 0) {}
    const unsigned n = g_trace_n < MI_TRACE_N ? g_trace_n : MI_TRACE_N;
    for (unsigned i = 0; i < n; i++) {
        const char *s = g_trace[(g_trace_n - n + i) % MI_TRACE_N];
        if (s && (write(2, "  ", 2) < 0 || write(2, s, strlen(s)) < 0 || write(2, "\n", 1) < 0)) {}
    }
    signal(sig, g_trace_prev == SIG_IGN || g_trace_prev == SIG_ERR ? SIG_DFL : g_trace_prev);
    raise(sig);
}
static int mi_trace_enabled(void) {
    if (g_trace_on < 0) {
        const char *e = getenv("RESNET_MI_TRACE");
        g_trace_on = e && atoi(e) ? 1 : 0;
        if (g_trace_on && atoi(e) > 1) fprintf(stderr, "resnet_mi: launch trace on\n");
    }
    return g_trace_on;
}
// ---- LDS fill after every launch (test aid, off unless mi_debug_lds_fill_mode or RESNET_MI_LDS_FILL=<hex word>) ----
// LDS is not cleared between dispatches: a kernel that reads an LDS word it never wrote reads what its predecessor on that CU left there.
// While the mode is on, every kernel launch of the library is followed by device synchronise, one word into every LDS word of every CU
// (mid_lds_fill), device synchronise -- so every kernel, not only the first of an operator or a step, finds that word in all LDS it does not
// write itself.  The fill's workgroups own LDS of their own, so the mode only serialises the launches; it changes no value.
static std::mutex g_lds_mu;                      /* the loader's prefetch thread launches too */
static std::atomic<int> g_lds_on{-1};            /* -1: the environment has not been read yet */
static uint32_t g_lds_word = 0;
static std::atomic<size_t> g_lds_fills{0};
static int lds_mode_on(void) {
    int on = g_lds_on.load(std::memory_order_acquire);
    if (on >= 0) return on;
    std::lock_guard<std::mutex> lk(g_lds_mu);
    if (g_lds_on < 0) {
        const char *e = getenv("RESNET_MI_LDS_FILL");
        if (e && *e) g_lds_word = (uint32_t)strtoul(e, NULL, 16);
        g_lds_on = e && *e ? 1 : 0;
    }
    return g_lds_on;
}
static void lds_fill_after_launch(void) {
    if (hipPeekAtLastError() != hipSuccess) return; /* the launch failed: its error stays for MI_LAUNCH_CHECK */
    std::lock_guard<std::mutex> lk(g_lds_mu);
    if (g_lds_on != 1) return;                      /* switched off meanwhile */
    if (mid_lds_fill(g_lds_word) == 0) g_lds_fills++; /* launches its kernel without MI_LAUNCH_CHECK: no way back into here */
}
void mi_trace_launch(const char *name) {
    if (mi_trace_enabled()) {
        g_trace[g_trace_n++ % MI_TRACE_N] = name;
        /* others (Python's faulthandler, test runners) install SIGABRT handlers of their own later on: stay in front of them */
        struct sigaction cur;
        if (sigaction(SIGABRT, NULL, &cur) == 0 && cur.sa_handler != mi_trace_dump) {
            g_trace_prev = (cur.sa_flags & SA_SIGINFO) ? SIG_DFL : cur.sa_handler;
            signal(SIGABRT, mi_trace_dump);
        }
    }
    if (lds_mode_on()) lds_fill_after_launch(); /* after the ring has the name: a fault the synchronise meets is dumped with it */
}
extern "C" {
int mid_debug_lds_fill(uint32_t word) {
    std::lock_guard<std::mutex> lk(g_lds_mu);
    return mid_lds_fill(word);
}
int mid_debug_lds_probe(uint32_t word, size_t out[4]) {
    std::lock_guard<std::mutex> lk(g_lds_mu);
    return mid_lds_probe(word, out);
}
int mid_debug_lds_geometry(size_t out[3]) {
    std::lock_guard<std::mutex> lk(g_lds_mu);
    return mid_lds_geometry(out);
}
/* on: fills LDS once at once, so that the first launch under the mode finds the word too; the counter starts at zero */
int mid_debug_lds_fill_mode(int on, uint32_t word) {
    lds_mode_on(); /* the environment is read before the first explicit setting, never after it */
    std::lock_guard<std::mutex> lk(g_lds_mu);
    g_lds_on = 0;
    if (!on) return 0;
    if (mid_lds_fill(word)) return -1;
    g_lds_word = word;
    g_lds_fills = 0;
    g_lds_on = 1;
    return 0;
}
size_t mid_debug_lds_fills(void) { return g_lds_fills; }
}
/* variant names: each distinct one is stored once and never moves (the ring and the abort dump keep pointers) */
#define MI_NAME_MAX 512
#define MI_NAME_LEN 96
static char g_names[MI_NAME_MAX][MI_NAME_LEN];
static int g_names_n = 0;
static std::mutex g_names_mu;
const char *mi_trace_name(const char *fmt, ...) {
    if (!mi_trace_enabled()) return fmt;
    char buf[MI_NAME_LEN];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(g_names_mu);
    for (int i = 0; i < g_names_n; i++)
        if (!strcmp(g_names[i], buf)) return g_names[i];
    if (g_names_n == MI_NAME_MAX) return fmt;
    memcpy(g_names[g_names_n], buf, sizeof buf);
    return g_names[g_names_n++];
}
extern "C" {
/* the ring's names, oldest first, one per line (what fits in cap bytes, always terminated); returns how many the ring holds */
int mid_trace_names(char *buf, size_t cap) {
    const unsigned n = g_trace_n < MI_TRACE_N ? g_trace_n : MI_TRACE_N;
    size_t at = 0;
    if (buf && cap) buf[0] = 0;
    for (unsigned i = 0; i < n; i++) {
        const char *s = g_trace[(g_trace_n - n + i) % MI_TRACE_N];
        const size_t l = s ? strlen(s) : 0;
        if (!buf || at + l + 2 > cap) continue;
        memcpy(buf + at, s, l);
        buf[at + l] = '\n'; buf[at + l + 1] = 0;
        at += l + 1;
    }
    return (int)n;
}
void mid_trace_clear(void) { g_trace_n = 0; }
}
#define HIPCHK(x)                                                          \
    do {                                                                   \
        hipError_t e_ = (x);                                               \
        if (e_ != hipSuccess) mi_record_error(#x, hipGetErrorString(e_)); \
    } while (0)

// ---- red-zone mode of the device allocator (test aid, off by default: mi_debug_redzone) ----
// While it is on, b bytes are allocated as zone | b | zone, all of it filled with one byte value; the zones are compared with that value
// when the allocation is freed and in mid_redzone_check.  Every access stays inside the process's own allocations.
struct RzEntry { char *user; size_t bytes, zone; int fill; unsigned long serial; bool damaged; };
static std::mutex g_rz_mu;                       /* the loader's prefetch thread allocates too */
static std::vector<RzEntry> g_rz;                /* live padded allocations */
static std::atomic<size_t> g_rz_zone{0}, g_rz_live{0};
static int g_rz_fill = 0, g_rz_damaged = 0;
static unsigned long g_rz_serial = 0;
static size_t g_rz_checked_allocs = 0, g_rz_checked_bytes = 0;
static char g_rz_first[320] = "";
static void *rz_malloc(size_t bytes) {
    std::lock_guard<std::mutex> lk(g_rz_mu);
    const size_t zone = g_rz_zone;
    if (!zone) { /* switched off meanwhile */
        void *q = nullptr;
        hipError_t e0 = hipMalloc(&q, bytes);
        if (e0 != hipSuccess) { mi_record_error("hipMalloc", hipGetErrorString(e0)); return nullptr; }
        return q;
    }
    char *base = nullptr;
    hipError_t e = hipMalloc((void **)&base, bytes + 2 * zone);
    if (e != hipSuccess) { mi_record_error("hipMalloc", hipGetErrorString(e)); return nullptr; }
    HIPCHK(hipMemsetAsync(base, g_rz_fill, bytes + 2 * zone, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr)); /* the fill is complete before the pointer is used on any stream */
    g_rz.push_back(RzEntry{base + zone, bytes, zone, g_rz_fill, ++g_rz_serial, false});
    g_rz_live = g_rz.size();
    return base + zone;
}
/* compares both zones of e with its fill (the caller holds the lock and has synchronised the device) */
static void rz_verify(RzEntry &e) {
    std::vector<unsigned char> h(e.zone);
    g_rz_checked_allocs++;
    for (int side = 0; side < 2; side++) {
        const char *z = side ? e.user + e.bytes : e.user - e.zone;
        if (hipMemcpy(h.data(), z, e.zone, hipMemcpyDeviceToHost) != hipSuccess) { mi_record_error("mi_debug_redzone", "copy of a zone failed"); return; }
        g_rz_checked_bytes += e.zone;
        size_t n = 0, first = 0, last = 0;
        for (size_t i = 0; i < e.zone; i++)
            if (h[i] != (unsigned char)e.fill) { if (!n++) first = i; last = i; }
        if (!n) continue;
        if (!e.damaged) { e.damaged = true; g_rz_damaged++; }
        if (!g_rz_first[0]) {
            /* offsets: back zone from the payload's end (0 = the first byte behind it), front zone from its start (-1 = the byte before it) */
            const long off = side ? 0 : -(long)e.zone;
            snprintf(g_rz_first, sizeof g_rz_first, "mi_debug_redzone: red zone damaged: allocation #%lu of %zu bytes, %s zone, offsets %ld..%ld from the payload's %s, %zu bytes "
                     "(fill 0x%02x, first damaged byte 0x%02x)", e.serial, e.bytes, side ? "back" : "front", (long)first + off, (long)last + off,
                     side ? "end" : "start", n, e.fill, h[first]);
            if (g_err[0] == 0) snprintf(g_err, sizeof g_err, "%s", g_rz_first);
        }
    }
}
/* 1: p was a padded allocation (verified and freed) */
static int rz_free(void *p) {
    std::lock_guard<std::mutex> lk(g_rz_mu);
    for (size_t i = 0; i < g_rz.size(); i++) {
        if (g_rz[i].user != (char *)p) continue;
        HIPCHK(hipDeviceSynchronize());
        rz_verify(g_rz[i]);
        HIPCHK(hipFree(g_rz[i].user - g_rz[i].zone));
        g_rz[i] = g_rz.back();
        g_rz.pop_back();
        g_rz_live = g_rz.size();
        return 1;
    }
    return 0;
}

extern "C" {
const char *mid_last_error(void) { return g_err; }
void mid_clear_error(void) { g_err[0] = 0; }
void mi_record_host_error(const char *what, const char *detail) { mi_record_error(what, detail); }
int mid_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int mid_set_device(int dev) {
    hipError_t e = hipSetDevice(dev);
    if (e != hipSuccess) { mi_record_error("hipSetDevice", hipGetErrorString(e)); return -1; }
    return 0;
}
void *mid_malloc(size_t bytes) {
    if (!bytes) bytes = 4;
    if (g_rz_zone) return rz_malloc(bytes);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) { mi_record_error("hipMalloc", hipGetErrorString(e)); return nullptr; }
    return p;
}
void mid_free(void *p) {
    if (!p) return;
    if (g_rz_live && rz_free(p)) return;
    HIPCHK(hipFree(p));
}
/* red-zone mode of the allocator (test aid): zone_bytes == 0 off; else a multiple of 4096 (pointers keep hipMalloc's alignment; -1 otherwise).
 * Switching it on starts a new count of damaged allocations; allocations made under an earlier setting stay padded and checked */
int mid_redzone(size_t zone_bytes, int fill_byte) {
    if (zone_bytes % 4096) { mi_record_error("mi_debug_redzone", "zone_bytes is 0 or a multiple of 4096"); return -1; }
    std::lock_guard<std::mutex> lk(g_rz_mu);
    g_rz_zone = zone_bytes;
    g_rz_fill = fill_byte & 0xff;
    if (zone_bytes) {
        g_rz_damaged = 0; g_rz_checked_allocs = g_rz_checked_bytes = 0; g_rz_first[0] = 0;
        for (RzEntry &e : g_rz) e.damaged = false;
    }
    return 0;
}
/* verifies the zones of every live padded allocation after a device synchronise; returns the number of damaged allocations seen since the mode
 * was last switched on (those found at mid_free included); the first one is described in mid_last_error */
int mid_redzone_check(void) {
    std::lock_guard<std::mutex> lk(g_rz_mu);
    if (!g_rz.empty()) HIPCHK(hipDeviceSynchronize());
    for (RzEntry &e : g_rz) rz_verify(e);
    if (g_rz_damaged && g_rz_first[0] && g_err[0] == 0) snprintf(g_err, sizeof g_err, "%s", g_rz_first); /* the channel was cleared since */
    return g_rz_damaged;
}
/* allocations verified and zone bytes compared since the mode was last switched on, and the padded allocations live now */
void mid_redzone_stats(size_t *allocs_checked, size_t *zone_bytes_checked, size_t *live) {
    std::lock_guard<std::mutex> lk(g_rz_mu);
    if (allocs_checked) *allocs_checked = g_rz_checked_allocs;
    if (zone_bytes_checked) *zone_bytes_checked = g_rz_checked_bytes;
    if (live) *live = g_rz.size();
}
void *mid_malloc_host(size_t bytes) {
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 4, hipHostMallocDefault);
    if (e != hipSuccess) { mi_record_error("hipHostMalloc", hipGetErrorString(e)); return nullptr; }
    return p;
}
void mid_free_host(void *p) { if (p) HIPCHK(hipHostFree(p)); }
void mid_memcpy_h2d(void *d, const void *s, size_t n, mid_stream st) { HIPCHK(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, (hipStream_t)st)); }
void mid_memcpy_d2h(void *d, const void *s, size_t n, mid_stream st) { HIPCHK(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, (hipStream_t)st)); }
void mid_memcpy_d2d(void *d, const void *s, size_t n, mid_stream st) { HIPCHK(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, (hipStream_t)st)); }
void mid_memset(void *d, int b, size_t n, mid_stream st) { HIPCHK(hipMemsetAsync(d, b, n, (hipStream_t)st)); }
mid_stream mid_stream_create(void) {
    hipStream_t s = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return (mid_stream)s;
}
/* a stream whose workgroups are dispatched only when the normal-priority streams leave capacity */
mid_stream mid_stream_create_low_priority(void) {
    int lo = 0, hi = 0;
    hipStream_t s = nullptr;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = 0; }
    HIPCHK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, lo)); /* numerically greatest = lowest priority */
    return (mid_stream)s;
}
void mid_stream_destroy(mid_stream s) { if (s) HIPCHK(hipStreamDestroy((hipStream_t)s)); }
void mid_stream_sync(mid_stream s) { HIPCHK(hipStreamSynchronize((hipStream_t)s)); }
void mid_device_sync(void) { HIPCHK(hipDeviceSynchronize()); }
mid_event mid_event_create(void) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreate(&e));
    return (mid_event)e;
}
void mid_event_destroy(mid_event e) { if (e) HIPCHK(hipEventDestroy((hipEvent_t)e)); }
void mid_event_record(mid_event e, mid_stream s) { HIPCHK(hipEventRecord((hipEvent_t)e, (hipStream_t)s)); }
void mid_stream_wait_event(mid_stream s, mid_event e) { HIPCHK(hipStreamWaitEvent((hipStream_t)s, (hipEvent_t)e, 0)); }
void mid_event_sync(mid_event e) { HIPCHK(hipEventSynchronize((hipEvent_t)e)); }
float mid_event_elapsed_ms(mid_event a, mid_event b) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, (hipEvent_t)a, (hipEvent_t)b));
    return ms;
}

} // extern "C"

// ---------------- per-family kernel timing ----------------
#define PROF_MAX 8192
static struct {
    int on, n, open;
    hipEvent_t a[PROF_MAX], b[PROF_MAX];
    int fam[PROF_MAX];
    long launches[MI_FAM_COUNT];
    double ms[MI_FAM_COUNT], flops[MI_FAM_COUNT], bytes[MI_FAM_COUNT];
    int created;
} P;
static void prof_resolve(void) {
    for (int i = 0; i < P.n; i++) {
        float ms = 0;
        if (hipEventSynchronize(P.b[i]) == hipSuccess && hipEventElapsedTime(&ms, P.a[i], P.b[i]) == hipSuccess) P.ms[P.fam[i]] += ms;
    }
    P.n = 0;
}
void mi_prof_begin(hipStream_t st, int fam, double flops, double bytes) {
    if (!(P.on & (1 << fam))) return;
    if (P.n == PROF_MAX) prof_resolve();
    const int i = P.n;
    if (i >= P.created) { HIPCHK(hipEventCreate(&P.a[i])); HIPCHK(hipEventCreate(&P.b[i])); P.created = i + 1; }
    P.fam[i] = fam; P.launches[fam]++; P.flops[fam] += flops; P.bytes[fam] += bytes;
    HIPCHK(hipEventRecord(P.a[i], st));
    P.open = 1;
}
void mi_prof_end(hipStream_t st) {
    if (!P.on || !P.open) return;
    HIPCHK(hipEventRecord(P.b[P.n], st));
    P.n++; P.open = 0;
}
extern "C" {
void mid_prof_enable(int on) { P.on = on == 1 ? 0xff : on; } /* 1 = all families, else a bit mask (1 << family) */
void mid_prof_reset(void) {
    prof_resolve();
    for (int f = 0; f < MI_FAM_COUNT; f++) { P.launches[f] = 0; P.ms[f] = P.flops[f] = P.bytes[f] = 0; }
}
void mid_prof_get(int family, long *launches, double *ms, double *flops, double *bytes) {
    prof_resolve();
    if (family < 0 || family >= MI_FAM_COUNT) return;
    if (launches) *launches = P.launches[family];
    if (ms) *ms = P.ms[family];
    if (flops) *flops = P.flops[family];
    if (bytes) *bytes = P.bytes[family];
}
}

extern "C" {
// ---------------- RCCL through dlopen: no link-time dependency, one copy per process ----------------
typedef struct { char internal[128]; } rcclUniqueId;
typedef int (*fn_getuid)(rcclUniqueId *);
typedef int (*fn_cominit)(void **, int, rcclUniqueId, int);
typedef int (*fn_allreduce)(const void *, void *, size_t, int, int, void *, hipStream_t);
typedef int (*fn_destroy)(void *);
typedef const char *(*fn_errstr)(int);
static struct { void *h; fn_getuid getuid; fn_cominit init; fn_allreduce allreduce; fn_destroy destroy; fn_destroy abort; fn_errstr errstr; } R;
static int rccl_load(void) {
    if (R.h) return 0;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (int i = 0; i < 3 && !R.h; i++) R.h = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
    if (!R.h) { mi_record_error("dlopen(librccl)", dlerror()); return -1; }
    R.getuid = (fn_getuid)dlsym(R.h, "ncclGetUniqueId");
    R.init = (fn_cominit)dlsym(R.h, "ncclCommInitRank");
    R.allreduce = (fn_allreduce)dlsym(R.h, "ncclAllReduce");
    R.destroy = (fn_destroy)dlsym(R.h, "ncclCommDestroy");
    R.abort = (fn_destroy)dlsym(R.h, "ncclCommAbort");
    R.errstr = (fn_errstr)dlsym(R.h, "ncclGetErrorString");
    if (!R.getuid || !R.init || !R.allreduce || !R.destroy) { mi_record_error("dlsym(rccl)", "missing symbol"); return -1; }
    return 0;
}
#define RCCLCHK(x, what)                                                               \
    do {                                                                               \
        int r_ = (x);                                                                  \
        if (r_ != 0) { mi_record_error(what, R.errstr ? R.errstr(r_) : "rccl error"); return -1; } \
    } while (0)
int mid_rccl_unique_id_bytes(void) { return (int)sizeof(rcclUniqueId); }
int mid_rccl_get_unique_id(void *out, int bytes) {
    if (bytes < (int)sizeof(rcclUniqueId) || rccl_load()) return -1;
    rcclUniqueId id;
    RCCLCHK(R.getuid(&id), "ncclGetUniqueId");
    memcpy(out, &id, sizeof id);
    return 0;
}
void *mid_rccl_comm_init(int rank, int world, const void *uid, int bytes) {
    if (bytes < (int)sizeof(rcclUniqueId) || rccl_load()) return nullptr;
    rcclUniqueId id;
    memcpy(&id, uid, sizeof id);
    void *comm = nullptr;
    int r = R.init(&comm, world, id, rank);
    if (r != 0) { mi_record_error("ncclCommInitRank", R.errstr ? R.errstr(r) : "rccl error"); return nullptr; }
    return comm;
}
int mid_rccl_allreduce_sum(void *comm, float *buf, size_t count, mid_stream s) {
    /* ncclFloat32 = 7, ncclSum = 0; in place */
    RCCLCHK(R.allreduce(buf, buf, count, 7, 0, comm, (hipStream_t)s), "ncclAllReduce");
    return 0;
}
void mid_rccl_comm_destroy(void *comm) { if (comm && R.destroy) R.destroy(comm); }
/* a rank that is about to exit on an error: tears the communicator down so that its peers' collectives fail instead of hanging */
void mid_rccl_comm_abort(void *comm) { if (comm && R.abort) R.abort(comm); }
}
