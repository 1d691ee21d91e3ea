// b64x_sessions.cpp -- the host's resource management behind include/b64x.h:
// thread placement, sessions (streams, pinned buffers, the pool, the
// in-place/staged policy), pinned allocations and the hub's batch lanes.
// Host code only: compiled without a device pass, it holds no kernel and
// launches none.  The kernels its calls end in, and their launchers, live in
// b64x_kernels.hip behind b64x_launch.h, so no change here can change GPU
// code.
#include <hip/hip_runtime_api.h>

#include <errno.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <atomic>
#include <mutex>

#include "b64x.h"
#include "b64x_launch.h"
#include "b64x_result_check.h"

using namespace b64x_launch;

extern "C" {

// ---- host placement (sysfs; no libnuma in the image) ----------------------

static bool read_small(const char *path, char *buf, size_t cap)
{
    FILE *f = fopen(path, "r");
    if (!f) return false;
    const size_t n = fread(buf, 1, cap - 1, f);
    fclose(f);
    buf[n] = 0;
    return n > 0;
}

int b64x_device_numa_node(int device)
{
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return -ENODEV;
    char bus[64];
    if (hipDeviceGetPCIBusId(bus, (int) sizeof bus, device) != hipSuccess) return -ENODEV;
    for (char *c = bus; *c; c++)
        if (*c >= 'A' && *c <= 'F') *c = (char) (*c - 'A' + 'a');
    char path[160], v[32];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    if (!read_small(path, v, sizeof v)) return -ENOENT;
    const int node = atoi(v);
    return node >= 0 ? node : -ENOENT;
}

// "0-63,128-191" -> set
static bool parse_cpulist(const char *s, cpu_set_t *set)
{
    CPU_ZERO(set);
    bool any = false;
    while (*s) {
        char *e = nullptr;
        long a = strtol(s, &e, 10);
        if (e == s) break;
        long b = a;
        s = e;
        if (*s == '-') {
            b = strtol(s + 1, &e, 10);
            s = e;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++) {
            CPU_SET((int) c, set);
            any = true;
        }
        while (*s == ',' || *s == '\n' || *s == ' ') s++;
    }
    return any;
}

int b64x_bind_thread(int device)
{
    const int node = b64x_device_numa_node(device);
    if (node < 0) return node;
    char path[96], list[4096];
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    cpu_set_t on_node, mine, both;
    if (!read_small(path, list, sizeof list) || !parse_cpulist(list, &on_node)) return -ENOENT;
    if (sched_getaffinity(0, sizeof mine, &mine) != 0) return -errno;
    CPU_AND(&both, &on_node, &mine);
    if (CPU_COUNT(&both) == 0) return -ENOENT;  // the thread may not run there
    if (CPU_EQUAL(&both, &mine)) return node;   // already inside the node
    // a mask inside another single node: the application placed the thread
    bool one_node = true;
    int first = -1;
    for (int c = 0; c < CPU_SETSIZE && one_node; c++) {
        if (!CPU_ISSET(c, &mine)) continue;
        char np[96];
        int n = -1;
        for (int k = 0; k < 64 && n < 0; k++) {
            snprintf(np, sizeof np, "/sys/devices/system/cpu/cpu%d/node%d", c, k);
            if (access(np, F_OK) == 0) n = k;
        }
        if (first < 0) first = n;
        else if (n != first) one_node = false;
    }
    if (one_node) return first;
    if (sched_setaffinity(0, sizeof both, &both) != 0) return -errno;
    // prefer the node for the pages this thread faults in from now on
    unsigned long mask[16] = {0};
    if (node < 64 * 16) {
        mask[node / 64] = 1ul << (node % 64);
        (void) syscall(SYS_set_mempolicy, 1 /* MPOL_PREFERRED */, mask, (unsigned long) 64 * 16);
    }
    return node;
}

// ------------------------------------------------------------- sessions --

struct b64x_session {
    int device;
    hipStream_t stream;
    uint64_t cap;
    uint8_t *h_in, *h_out;
    uint8_t *h_base;     // h_in - kSessionHead (pinned, for in-place decodes)
    uint8_t *d_base;     // d_in - kSessionHead
    uint64_t last_len;   // characters of the last decode (0: none yet)
    bool dec_staged;     // the last decode found junk throughout: stage the next
    uint64_t res_len;    // characters, flags and sequence number of the last
    unsigned res_flags;  // decode, for the result check
    uint32_t res_seq;    // (b64x_session_decode_result)
    uint8_t *d_in, *d_out;
    void *d_ws;
    b64x_dec_result *d_res, *h_res;
};

// ---- completion results: written by the kernels, checked by the host ----
//
// A session decode's result record is written by the kernel that computes
// it straight into the fine-grained host mirror (no D2H copy behind the
// kernels), the host poisons the mirror before every launch, and
// b64x_session_decode_result() checks every field: a record that is still
// poisoned or inconsistent is counted, the session's stream is waited for,
// and the record is checked again (-EIO if it is still wrong: loud, never a
// silently short stream).  The hub's lanes do the same for their batches
// (b64x_lane_*_check).  Round 1 read records that D2H copies had filled, and
// under load (600 decoder streams on one loop on per-stage sessions) a block
// was now and then served as empty from a well-formed "nothing decoded"
// record (profiles/r02_diag_notes.md).  The check itself is
// b64x_result_check.h, shared with the CPU stage tests.
static std::atomic<uint64_t> g_early_session{0}, g_early_lane{0};

// Device headroom in front of d_in (kept for the decode kernels' vector
// loads, which may start below an unaligned input).
constexpr uint64_t kSessionHead = 256;
// Pinned slack after host_in: the decode kernels' last vector loads may
// reach past the input, harmless in a page-rounded hipMalloc, not assumed
// of host memory read in place.
constexpr uint64_t kSessionTail = 64;

static uint64_t session_out_cap(uint64_t cap)
{
    uint64_t e = b64x_encoded_len(cap, true), dcap = b64x_decoded_cap(cap);
    return e > dcap ? e : dcap;
}

// A session's pinned buffers are fine-grained (hipHostMallocCoherent).
// host_in/host_out are read and written in place by the kernels (zero-copy),
// and host_res is the target of the last small D2H copy before the
// completion callback once the output copy is gone; fine-grained memory is
// never held in an XCD's L2, so no fence scope can leave the host a stale
// line.  Defensive: the rates are unchanged (resident decode blocks 28.1 ->
// 27.8, encode 31.0 -> 30.9 GiB/s).  It did NOT cure the intermittent
// missing-block bug of the 600-stream decoder ingress (known
// issues; tests/tools/stress_ingress.py).
constexpr unsigned kSessionHostFlags = hipHostMallocCoherent;

b64x_session *b64x_session_open(uint64_t capacity)
{
    if (capacity == 0) {
        errno = EINVAL;
        return nullptr;
    }
    if (b64x_device_check() != 0) {
        errno = ENODEV;
        return nullptr;
    }
    b64x_session *s = (b64x_session *) calloc(1, sizeof(*s));
    if (!s) return nullptr;
    s->cap = capacity;
    (void) hipGetDevice(&s->device);
    const uint64_t ocap = session_out_cap(capacity);
    const uint64_t wsz = b64x_decode_workspace_size(capacity);
    bool ok = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) == hipSuccess &&
              hipHostMalloc((void **) &s->h_base, kSessionHead + capacity + kSessionTail,
                            kSessionHostFlags) == hipSuccess &&
              hipHostMalloc((void **) &s->h_out, ocap, kSessionHostFlags) == hipSuccess &&
              hipHostMalloc((void **) &s->h_res, sizeof(b64x_dec_result), kSessionHostFlags) == hipSuccess &&
              hipMalloc((void **) &s->d_base, kSessionHead + capacity) == hipSuccess &&
              hipMalloc((void **) &s->d_out, ocap) == hipSuccess &&
              hipMalloc((void **) &s->d_res, sizeof(b64x_dec_result)) == hipSuccess &&
              hipMalloc(&s->d_ws, wsz) == hipSuccess &&
              hipMemset(s->d_ws, 0, wsz) == hipSuccess;
    if (!ok) {
        b64x_session_close(s);
        errno = ENOMEM;
        return nullptr;
    }
    s->d_in = s->d_base + kSessionHead;
    s->h_in = s->h_base + kSessionHead;
    return s;
}

void b64x_session_close(b64x_session *s)
{
    if (!s) return;
    int prev = 0;
    (void) hipGetDevice(&prev);
    (void) hipSetDevice(s->device);
    if (s->stream) (void) hipStreamSynchronize(s->stream);
    if (s->h_base) (void) hipHostFree(s->h_base);
    if (s->h_out) (void) hipHostFree(s->h_out);
    if (s->h_res) (void) hipHostFree(s->h_res);
    if (s->d_base) (void) hipFree(s->d_base);
    if (s->d_out) (void) hipFree(s->d_out);
    if (s->d_res) (void) hipFree(s->d_res);
    if (s->d_ws) (void) hipFree(s->d_ws);
    if (s->stream) (void) hipStreamDestroy(s->stream);
    (void) hipSetDevice(prev);
    free(s);
}

uint64_t b64x_session_capacity(const b64x_session *s) { return s ? s->cap : 0; }

// Idle sessions, any device / capacity; at most kPoolMax kept.
static std::mutex g_pool_mu;
static b64x_session *g_pool[64];
static int g_npool;
constexpr int kPoolMax = 64;

static bool pool_enabled()
{
    static const bool on = [] {
        const char *v = getenv("ASYNC_B64_SESSION_POOL");
        return !(v && v[0] == '0');
    }();
    return on;
}

b64x_session *b64x_session_acquire(uint64_t capacity)
{
    int dev = 0;
    if (pool_enabled() && hipGetDevice(&dev) == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (int i = g_npool - 1; i >= 0; i--) {
            b64x_session *s = g_pool[i];
            if (s->device == dev && s->cap == capacity) {
                g_pool[i] = g_pool[--g_npool];
                return s;
            }
        }
    }
    return b64x_session_open(capacity);
}

void b64x_session_release(b64x_session *s)
{
    if (!s) return;
    if (pool_enabled() && b64x_session_wait(s) == 0) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (g_npool < kPoolMax) {
            g_pool[g_npool++] = s;
            return;
        }
    }
    b64x_session_close(s);
}
uint8_t *b64x_session_host_in(b64x_session *s) { return s ? s->h_in : nullptr; }
uint8_t *b64x_session_host_out(b64x_session *s) { return s ? s->h_out : nullptr; }

int b64x_session_encode(b64x_session *s, uint64_t n, const b64x_alphabet *abc,
                        uint64_t *out_len)
{
    if (!s || n > s->cap || !out_len) return -EINVAL;
    *out_len = 0;
    int err;
    if ((err = b64x_session_encode_async(s, n, abc, nullptr, nullptr))) return err;
    if ((err = b64x_session_wait(s))) return err;
    *out_len = n ? b64x_encoded_len(n, abc ? abc->pad : true) : 0;
    return 0;
}

int b64x_session_decode(b64x_session *s, uint64_t n, const b64x_alphabet *abc,
                        unsigned flags, b64x_dec_result *res)
{
    if (!s || n > s->cap || !res) return -EINVAL;
    memset(res, 0, sizeof(*res));
    int err;
    if ((err = b64x_session_decode_async(s, n, abc, flags, nullptr, nullptr))) return err;
    if ((err = b64x_session_wait(s))) return err;
    return b64x_session_decode_result(s, res);
}

// A session's encode reads and writes its pinned host buffers in place over
// PCIe (zero-copy) instead of H2D, kernel, D2H: each byte crosses PCIe once
// either way, but one kernel's reads and writes overlap (duplex) and nothing
// is staged through HBM -- 30 GiB/s of payload against 22 staged for 32 MiB
// blocks (bench_host_pipeline resident_encode; scripts/bench_zero_copy.py).
// Not for the hub's ragged batches: one block per job is PCIe-latency-bound
// in place (a single 1 MiB stream ran at half the staged rate).
// ASYNC_B64_ZERO_COPY=0 stages sessions too.
static bool zero_copy_sessions()
{
    static const bool on = [] {
        const char *v = getenv("ASYNC_B64_ZERO_COPY");
        return !(v && v[0] == '0');
    }();
    return on;
}

int b64x_session_encode_async(b64x_session *s, uint64_t n, const b64x_alphabet *abc,
                              b64x_done_fn done, void *arg)
{
    if (!s || n > s->cap) return -EINVAL;
    int err;
    if ((err = hip_err(hipSetDevice(s->device)))) return err;
    if (n && zero_copy_sessions()) {
        if ((err = b64x_encode_dev(s->h_in, n, s->h_out, abc, s->stream))) return err;
    } else if (n) {
        const uint64_t m = b64x_encoded_len(n, abc ? abc->pad : true);
        if ((err = hip_err(hipMemcpyAsync(s->d_in, s->h_in, n, hipMemcpyHostToDevice, s->stream)))) return err;
        if ((err = b64x_encode_dev(s->d_in, n, s->d_out, abc, s->stream))) return err;
        if ((err = hip_err(hipMemcpyAsync(s->h_out, s->d_out, m, hipMemcpyDeviceToHost, s->stream)))) return err;
    }
    if (done) return hip_err(hipLaunchHostFunc(s->stream, done, arg));
    return 0;
}

// A session's decode reads host_in and writes host_out in place over PCIe
// too, unless its last decode found junk throughout (MIME line breaks):
// pass 2 re-reads the input and pass-1 output where junk is, which in place
// means a second PCIe crossing.  Clean 256 MiB blocks 22.6 -> 34.5 GiB/s,
// CRLF-76 ones 21.6 staged against 17.7 in place (scripts/bench_zero_copy.py).
// The result of the last decode is consulted only once the session's stream
// has drained, so the policy never waits and never reads a result in flight.
// ASYNC_B64_ZERO_COPY=0 stages every decode as well.
constexpr uint64_t kZeroCopyJunk = 80;  // skipped characters that make the next decode staged

static bool decode_in_place(b64x_session *s)
{
    if (!zero_copy_sessions()) return false;
    b64x_dec_result r;
    if (s->last_len && hipStreamQuery(s->stream) == hipSuccess &&
        b64x_result_ok(s->h_res, s->res_len, s->res_flags, s->res_seq, &r)) {
        const uint64_t junk = s->last_len - (r.valid < s->last_len ? r.valid : s->last_len);
        s->dec_staged = junk > kZeroCopyJunk;
        s->last_len = 0;
    }
    return !s->dec_staged;
}

// Round 1 chained a stream's blocks over sessions on the device (a carry
// spelled by a kernel on the previous session's stream, a cross-stream
// event, the record copied D2H behind the kernels), and a block was once in
// a while served as empty from a well-formed "nothing decoded" record.  That
// chaining is gone: a session decode is H2D (or in place),
// the kernels and the completion, all on the session's own stream, and the
// record the kernels write into host memory names this call (n, flags and
// a fresh sequence number), so no earlier or zero-filled record passes the
// check.
int b64x_session_decode_async(b64x_session *s, uint64_t n, const b64x_alphabet *abc,
                              unsigned flags, b64x_done_fn done, void *arg)
{
    if (!s || n > s->cap) return -EINVAL;
    int err;
    if ((err = hip_err(hipSetDevice(s->device)))) return err;
    const bool in_place = decode_in_place(s);
    uint8_t *in = in_place ? s->h_in : s->d_in;
    uint8_t *out = in_place ? s->h_out : s->d_out;
    if (n && !in_place &&
        (err = hip_err(hipMemcpyAsync(s->d_in, s->h_in, n, hipMemcpyHostToDevice, s->stream))))
        return err;
    b64x_poison_result(s->h_res);
    s->res_len = n;
    s->res_flags = flags;
    s->res_seq = next_seq();
    if ((err = decode_dev_impl(in, n, out, s->d_res, s->h_res, abc, flags, s->d_ws, s->stream,
                               s->res_seq)))
        return err;
    s->last_len = n;
    // The output length is device-determined: copy the capacity bound.
    if (n && !in_place &&
        (err = hip_err(hipMemcpyAsync(s->h_out, s->d_out, b64x_decoded_cap(n),
                                      hipMemcpyDeviceToHost, s->stream))))
        return err;
    if (done) return hip_err(hipLaunchHostFunc(s->stream, done, arg));
    return 0;
}

const b64x_dec_result *b64x_session_result(const b64x_session *s)
{
    return s ? s->h_res : nullptr;
}

int b64x_session_decode_result(b64x_session *s, b64x_dec_result *res)
{
    if (!s || !res) return -EINVAL;
    if (b64x_result_ok(s->h_res, s->res_len, s->res_flags, s->res_seq, res)) return 0;
    g_early_session.fetch_add(1, std::memory_order_relaxed);
    int err = b64x_session_wait(s);
    if (err) return err;
    const bool ok = b64x_result_ok(s->h_res, s->res_len, s->res_flags, s->res_seq, res);
    return ok ? 0 : -EIO;
}

void b64x_diag_counters(uint64_t out[2])
{
    out[0] = g_early_session.load(std::memory_order_relaxed);
    out[1] = g_early_lane.load(std::memory_order_relaxed);
}

int b64x_session_wait(b64x_session *s)
{
    if (!s) return -EINVAL;
    return hip_err(hipStreamSynchronize(s->stream));
}

// ------------------------------------------------------------ batch lanes --

void *b64x_host_alloc(uint64_t bytes)
{
    void *p = nullptr;
    if (b64x_device_check() != 0) return nullptr;
    // Fine-grained, like a session's buffers: a lane's decode batch ends on a
    // small D2H copy of the output lengths right before its host callback
    // (see kSessionHostFlags).
    if (hipHostMalloc(&p, bytes ? bytes : 1, kSessionHostFlags) != hipSuccess) return nullptr;
    return p;
}

void b64x_host_free(void *p)
{
    if (p) (void) hipHostFree(p);
}

// A lane's batches read their input from device memory (one H2D copy of the
// arena) and write their outputs -- characters, bytes and the decode jobs'
// result records -- straight into the pinned host arena: no D2H copy.  The
// host checks every batch once its completion callback has run: decode
// records were poisoned before the launch (b64x_lane_decode_check), and an
// encode batch ends with a kernel that stamps the lane's sequence number
// into host memory (b64x_lane_encode_check).  Round 1's D2H copies of
// results are what lost blocks under load.
struct b64x_lane {
    int device;
    hipStream_t stream;
    uint8_t *d_in;
    uint64_t *d_offs;     // in_off | out_off | vcount (decode) words
    uint8_t *d_flags;
    uint64_t *h_stamp;    // fine-grained pinned: the last finished encode batch
    uint64_t seq;         // the last encode batch queued
    uint64_t in_cap, offs_cap, flags_cap;  // bytes allocated
    b64x_seg *d_seg;      // an encode batch's lent segments (k_gather_host)
    uint64_t seg_cap;
    b64x_dec_result *d_res;  // big decode jobs: the pipeline's record ...
    void *d_ws;              // ... and workspace (allocated at the first)
};

b64x_lane *b64x_lane_open(void)
{
    if (b64x_device_check() != 0) {
        errno = ENODEV;
        return nullptr;
    }
    b64x_lane *l = (b64x_lane *) calloc(1, sizeof(*l));
    if (!l) return nullptr;
    (void) hipGetDevice(&l->device);
    if (hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking) != hipSuccess) {
        free(l);
        errno = EIO;
        return nullptr;
    }
    if (hipHostMalloc((void **) &l->h_stamp, sizeof(uint64_t), kSessionHostFlags) != hipSuccess) {
        (void) hipStreamDestroy(l->stream);
        free(l);
        errno = ENOMEM;
        return nullptr;
    }
    *l->h_stamp = 0;
    return l;
}

void b64x_lane_close(b64x_lane *l)
{
    if (!l) return;
    (void) hipSetDevice(l->device);
    (void) hipStreamSynchronize(l->stream);
    if (l->d_in) (void) hipFree(l->d_in);
    if (l->d_offs) (void) hipFree(l->d_offs);
    if (l->d_flags) (void) hipFree(l->d_flags);
    if (l->d_seg) (void) hipFree(l->d_seg);
    if (l->d_res) (void) hipFree(l->d_res);
    if (l->d_ws) (void) hipFree(l->d_ws);
    if (l->h_stamp) (void) hipHostFree(l->h_stamp);
    (void) hipStreamDestroy(l->stream);
    free(l);
}

static b64x_lane *g_lane_pool[64];
static int g_nlane_pool;

b64x_lane *b64x_lane_acquire(void)
{
    int dev = 0;
    if (pool_enabled() && hipGetDevice(&dev) == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (int i = g_nlane_pool - 1; i >= 0; i--) {
            b64x_lane *l = g_lane_pool[i];
            if (l->device == dev) {
                g_lane_pool[i] = g_lane_pool[--g_nlane_pool];
                return l;
            }
        }
    }
    return b64x_lane_open();
}

void b64x_lane_release(b64x_lane *l)
{
    if (!l) return;
    if (pool_enabled() && b64x_lane_wait(l) == 0) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (g_nlane_pool < kPoolMax) {
            g_lane_pool[g_nlane_pool++] = l;
            return;
        }
    }
    b64x_lane_close(l);
}

// Grow a device buffer to at least `need`, and on first use at least to
// `floor`: the size the hub's default batches need (16 MiB arenas, 2^16 jobs,
// 2^14 lent segments), so that a lane taken from the pool by another loop
// does not grow under load.  Growing synchronises the lane's stream and
// frees the old buffer (hipFree waits for the whole device); under config 5
// on 16 loops the lanes' growth and the arenas' allocation made passes
// 10-20 % slower now and then.
constexpr uint64_t kLaneInFloor = (16u << 20) + (1u << 20);
constexpr uint64_t kLaneOffsFloor = 3ull * ((1u << 16) + 1) * 8;
constexpr uint64_t kLaneFlagsFloor = (1u << 16) + 64;
constexpr uint64_t kLaneSegFloor = (1u << 14) * sizeof(b64x_seg);
static int lane_grow(b64x_lane *l, void **buf, uint64_t *cap, uint64_t need, uint64_t floor)
{
    if (need <= *cap) return 0;
    uint64_t want = need + need / 4 + (1u << 20);
    if (want < floor) want = floor;
    int err;
    if ((err = hip_err(hipStreamSynchronize(l->stream)))) return err;
    if (*buf) (void) hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    if (hipMalloc(buf, want) != hipSuccess) return -ENOMEM;
    *cap = want;
    return 0;
}

// Offsets (and, for decode, the per-job counts) and the input on the device
// (h_in NULL: the offsets only).
static int lane_stage_in(b64x_lane *l, const uint8_t *h_in, uint32_t njobs,
                         const uint64_t *h_in_off, const uint64_t *h_out_off, uint64_t words_extra)
{
    const uint64_t in_bytes = h_in_off[njobs];
    const uint64_t words = (uint64_t) njobs + 1;
    int err;
    if ((err = lane_grow(l, (void **) &l->d_in, &l->in_cap, in_bytes + 64, kLaneInFloor))) return err;
    if ((err = lane_grow(l, (void **) &l->d_offs, &l->offs_cap, (2 * words + words_extra) * 8,
                          kLaneOffsFloor)))
        return err;
    if ((err = hip_err(hipMemcpyAsync(l->d_offs, h_in_off, words * 8, hipMemcpyHostToDevice,
                                      l->stream))) ||
        (err = hip_err(hipMemcpyAsync(l->d_offs + words, h_out_off, words * 8,
                                      hipMemcpyHostToDevice, l->stream))))
        return err;
    if (h_in && in_bytes && (err = hip_err(hipMemcpyAsync(l->d_in, h_in, in_bytes,
                                                          hipMemcpyHostToDevice, l->stream))))
        return err;
    return 0;
}

int b64x_lane_encode_async(b64x_lane *l, const uint8_t *h_in, uint32_t njobs,
                           const uint64_t *h_in_off, uint8_t *h_out,
                           const uint64_t *h_out_off, const b64x_seg *h_seg, uint32_t nseg,
                           const b64x_alphabet *abc, b64x_done_fn done, void *arg)
{
    if (!l || (njobs && (!h_in || !h_in_off || !h_out || !h_out_off)) || (nseg && !h_seg))
        return -EINVAL;
    int err;
    if ((err = hip_err(hipSetDevice(l->device)))) return err;
    if (njobs) {
        const uint64_t words = (uint64_t) njobs + 1;
        const uint64_t in_bytes = h_in_off[njobs];
        for (uint32_t i = 0; i < nseg; i++)  // sorted, inside the batch (off + len may wrap)
            if (h_seg[i].len > in_bytes || h_seg[i].off > in_bytes - h_seg[i].len ||
                (i && h_seg[i].off < h_seg[i - 1].off + h_seg[i - 1].len))
                return -EINVAL;
        if ((err = lane_stage_in(l, nseg ? nullptr : h_in, njobs, h_in_off, h_out_off, 0)))
            return err;
        if (nseg && in_bytes) {
            if ((err = lane_grow(l, (void **) &l->d_seg, &l->seg_cap, (uint64_t) nseg * sizeof(b64x_seg),
                               kLaneSegFloor)) ||
                (err = hip_err(hipMemcpyAsync(l->d_seg, h_seg, (size_t) nseg * sizeof(b64x_seg),
                                              hipMemcpyHostToDevice, l->stream))))
                return err;
            if ((err = gather_host(l->d_in, h_in, in_bytes, l->d_seg, nseg, l->stream))) return err;
        }
        if ((err = b64x_encode_batch(l->d_in, l->d_offs, njobs, h_out, l->d_offs + words, abc,
                                     l->stream)))
            return err;
    }
    if ((err = stamp(l->h_stamp, ++l->seq, l->stream))) return err;
    if (done) return hip_err(hipLaunchHostFunc(l->stream, done, arg));
    return 0;
}

int b64x_lane_encode_check(b64x_lane *l)
{
    if (!l) return -EINVAL;
    if (*(volatile uint64_t *) l->h_stamp == l->seq) return 0;
    g_early_lane.fetch_add(1, std::memory_order_relaxed);
    int err = b64x_lane_wait(l);
    if (err) return err;
    return *(volatile uint64_t *) l->h_stamp == l->seq ? 0 : -EIO;
}

// Hub decode jobs this long go through the single-buffer pipeline.
static constexpr uint64_t kBigJob = 128u << 10;

int b64x_lane_decode_async(b64x_lane *l, const uint8_t *h_in, uint32_t njobs,
                           const uint64_t *h_in_off, uint8_t *h_out,
                           const uint64_t *h_out_off, const uint8_t *h_flags,
                           b64x_dec_result *h_res, const b64x_dec_result *const *h_prev,
                           b64x_dec_result *h_spell, const b64x_alphabet *abc,
                           b64x_done_fn done, void *arg, uint32_t *seq)
{
    if (!l || !seq || (njobs && (!h_in || !h_in_off || !h_out || !h_out_off || !h_flags || !h_res)))
        return -EINVAL;
    for (uint32_t j = 0; j < njobs; j++)
        if ((h_flags[j] & B64X_LANE_CHAINED) &&
            (!h_prev || !h_prev[j] || !h_spell || h_in_off[j + 1] - h_in_off[j] < 4))
            return -EINVAL;
    int err;
    if ((err = hip_err(hipSetDevice(l->device)))) return err;
    *seq = next_seq();
    if (njobs) {
        const uint64_t words = (uint64_t) njobs + 1;
        for (uint32_t j = 0; j < njobs; j++) b64x_poison_result(h_res + j);
        if ((err = lane_stage_in(l, h_in, njobs, h_in_off, h_out_off, words))) return err;
        if ((err = lane_grow(l, (void **) &l->d_flags, &l->flags_cap, njobs, kLaneFlagsFloor))) return err;
        if ((err = hip_err(hipMemcpyAsync(l->d_flags, h_flags, njobs, hipMemcpyHostToDevice,
                                          l->stream))))
            return err;
        uint64_t *d_in_off = l->d_offs, *d_out_off = l->d_offs + words,
                 *d_vcount = l->d_offs + 2 * words;
        // Jobs of kBigJob characters or more (whole stage blocks) would each
        // keep one wave of the batch kernel busy for hundreds of us: they
        // take the single-buffer pipeline instead, in job order on the lane's
        // stream, which writes their records itself; so do chained jobs,
        // whose heads are spelled between their predecessor's decode and
        // their own.  The batch kernels skip both.
        uint32_t npiped = 0;
        for (uint32_t j = 0; j < njobs; j++)
            npiped += h_in_off[j + 1] - h_in_off[j] >= kBigJob || (h_flags[j] & B64X_LANE_CHAINED);
        const uint8_t *src = h_in_off[njobs] ? l->d_in : (const uint8_t *) l->d_offs;
        if (npiped < njobs &&
            (err = lane_batch_decode(src, d_in_off, d_out_off, l->d_flags, njobs, kBigJob, h_out,
                                     d_vcount, h_res, abc, l->stream, *seq)))
            return err;
        if (npiped && !l->d_ws) {
            const uint64_t wsz = b64x_decode_workspace_size(0);
            if (!l->d_res && hipMalloc(&l->d_res, sizeof *l->d_res) != hipSuccess) {
                l->d_res = nullptr;
                return -ENOMEM;
            }
            if (hipMalloc(&l->d_ws, wsz) != hipSuccess) {
                l->d_ws = nullptr;
                return -ENOMEM;
            }
            if ((err = hip_err(hipMemsetAsync(l->d_ws, 0, wsz, l->stream)))) return err;
        }
        for (uint32_t j = 0; npiped && j < njobs; j++) {
            const uint64_t n = h_in_off[j + 1] - h_in_off[j];
            const bool chained = h_flags[j] & B64X_LANE_CHAINED;
            if (n < kBigJob && !chained) continue;
            if (chained && (err = spell_head(l->d_in + h_in_off[j], h_prev[j], h_spell + j, abc,
                                             l->stream)))
                return err;
            if ((err = decode_dev_impl(l->d_in + h_in_off[j], n, h_out + h_out_off[j], l->d_res,
                                       h_res + j, abc, h_flags[j] & 1 ? B64X_DEC_HOLD_TAIL : 0,
                                       l->d_ws, l->stream, *seq)))
                return err;
        }
    }
    if (done) return hip_err(hipLaunchHostFunc(l->stream, done, arg));
    return 0;
}

int b64x_lane_wait(b64x_lane *l)
{
    if (!l) return -EINVAL;
    return hip_err(hipStreamSynchronize(l->stream));
}

// Every record is this batch's and consistent; every chained job's head was
// spelled from its predecessor's finished record (checked before it: the
// predecessor is an earlier job of this batch or of a batch before it).
static bool jobs_ok(const uint64_t *h_in_off, const uint8_t *h_flags,
                    const b64x_dec_result *h_res, const b64x_dec_result *const *h_prev,
                    const b64x_dec_result *h_spell, uint32_t njobs, uint32_t seq)
{
    for (uint32_t j = 0; j < njobs; j++) {
        if (!b64x_result_ok(h_res + j, h_in_off[j + 1] - h_in_off[j], h_flags[j] & 1, seq,
                            nullptr))
            return false;
        if ((h_flags[j] & B64X_LANE_CHAINED) && !b64x_spell_ok(h_spell + j, h_prev[j]))
            return false;
    }
    return true;
}

int b64x_lane_decode_check(b64x_lane *l, uint32_t seq, const uint64_t *h_in_off,
                           const uint8_t *h_flags, const b64x_dec_result *h_res,
                           const b64x_dec_result *const *h_prev,
                           const b64x_dec_result *h_spell, uint32_t njobs)
{
    if (!l || (njobs && (!h_in_off || !h_flags || !h_res))) return -EINVAL;
    if (jobs_ok(h_in_off, h_flags, h_res, h_prev, h_spell, njobs, seq)) return 0;
    g_early_lane.fetch_add(1, std::memory_order_relaxed);
    int err = b64x_lane_wait(l);
    if (err) return err;
    return jobs_ok(h_in_off, h_flags, h_res, h_prev, h_spell, njobs, seq) ? 0 : -EIO;
}

}  // extern "C"
