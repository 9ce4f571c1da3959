// lt_api.hip -- host side of libltrace_hip.so: the C-ABI declared in include/ltrace.h.
//
// Everything here is plumbing around the three kernels of lt_kernels.hpp: build the
// wave-uniform constant blocks, size the grids, launch on the caller's stream, time with
// HIP events.  No CPU compute path exists: without a GPU the entry points fail.
#include "../../include/ltrace.h"
#include "lt_kernels.hpp"
#include "lt_disk.hpp"
#include "lt_disk_images.hpp"
#include "lt_hit_time.hpp"
#include "lt_hotspot.hpp"
#include "lt_polarization.hpp"
#include "lt_aa.hpp"
#include "lt_aa_adaptive.hpp"
#include "lt_hotspot_aa.hpp"
#include "lt_diskmap.hpp"
#include "lt_spectrum.hpp"
#include "lt_visibility.hpp"
#include "lt_visibility_stokes.hpp"
#include "lt_diskmovie.hpp"
#include "lt_thermal.hpp"
#ifdef LT_PROBES
#include "lt_probe.hpp"
#endif
#include "lt_dense.hpp"

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#ifndef LT_BUILD_ID
#define LT_BUILD_ID "unversioned"
#endif

using namespace lt;

// compiled in lt_k2_lone.hip (its own translation unit: another instruction scheduler, see there)
namespace lt {
extern template __global__ void k_kerr_direct<float, Rk4<float>>(KerrConsts<float>, const typename Vec4<float>::type *__restrict__,
                                                                 typename Vec4<float>::type *__restrict__, typename Vec4<float>::type *__restrict__,
                                                                 int64_t, uint32_t, uint4 *__restrict__, uint64_t *__restrict__, unsigned long long *__restrict__,
                                                                 int64_t);
}

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(LT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

extern "C" int lt_version(void) { return LT_VERSION; }
extern "C" const char *lt_build_id(void) { return LT_BUILD_ID; }
extern "C" const char *lt_last_error(void) { return g_err; }

extern "C" int lt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int lt_set_device(int device)
{
    if (lt_device_count() <= 0) return fail(LT_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    return LT_OK;
}

static int require_device()
{
    if (lt_device_count() <= 0)
        return fail(LT_ERR_NO_DEVICE, "libltrace_hip: no HIP device visible (this library has no CPU path)");
    return LT_OK;
}

// ---------------------------------------------------------------------------------------------
// per-device context.  Everything a call needs beyond the caller's own buffers is owned per
// (device, stream): the grow-only workspace of ray records, and for the host-pointer entry points
// the device-side inputs and outputs.  Two calls on different streams of one device
// therefore never share memory and may run concurrently; calls on the same stream are ordered by
// the stream.  Nothing is allocated per call once the buffers have grown to the frame size.
// ---------------------------------------------------------------------------------------------
struct EventQuad { hipEvent_t e[4]; };

struct Grow { // grow-only device allocation
    void *p = nullptr;
    size_t bytes = 0;
};

// What the ray records `ic` of a slot's workspace hold: every input k_prologue_camera reads, by value.  A frame whose
// key equals the slot's skips that launch -- the kernel would overwrite the records with the bytes they already hold.
// Only the records are reused: every frame still traces every ray and shades every pixel (K2, K3).
//   * Writers of `ic` are k_prologue_camera (render_dev_impl, which sets the key) and k_prologue_arrays (trace_batch);
//     the integrate kernels -- direct, queue and Schwarzschild, ghost lanes included, and both disks -- take `ic` as a
//     pointer to const and only load from it.
//   * Invalidation: get_workspace() clears the key for every caller and reports whether the buffer was replaced;
//     render_dev_impl sets it again once its prologue is enqueued, and clears it on any error return after that.
//     Releasing a slot deletes the key with it.
//   * Ordering: key and buffer belong to one StreamSlot, and all work of a slot is ordered by its stream, so a key set
//     at enqueue time describes the records every later launch on that stream will see.  Key accesses hold g_mu.
struct IcKey {
    bool valid = false;
    CamConsts cam{};              // zero-filled before its members are set, block_list cleared: compared with memcmp
    bool has_blocks = false;      // CamConsts::block_list != NULL ...
    std::vector<int32_t> blocks;  // ... and the host copy of what it points to
    int kind = 0, obs_ok = 0;     // MetricConsts: the members K1 reads
    double metric[15] = {};
    size_t elem = 0;              // record element size (float / double)
    int64_t n_q = 0;
    bool same(const IcKey &o) const
    {
        return valid && o.valid && memcmp(&cam, &o.cam, sizeof(cam)) == 0 && has_blocks == o.has_blocks && blocks == o.blocks &&
               kind == o.kind && obs_ok == o.obs_ok && memcmp(metric, o.metric, sizeof(metric)) == 0 && elem == o.elem &&
               n_q == o.n_q;
    }
};

struct StreamSlot {
    hipStream_t stream = nullptr;
    Grow ws;     // ray records of lt_render_dev / the batch twins
    IcKey ic_key; // what ws's `ic` holds (valid == false: nothing a frame may reuse)
    Grow dev;    // lt_render / batch twins: device-side inputs and outputs
    Grow dense;  // lt_integrate_dense_dev, length-binned launch: histogram, cursors, keys, permutation
    Grow blocks; // block-owner table mode: this partition's block list on the device
    Grow disk_img; // lt_render_disk_images / its batch twin: the integrate kernel's hit records and counts
    Grow disk_time; // lt_trace_disk_hits / its batch twin: the integrate kernel's hit times
    Grow disk_mom;  // lt_trace_disk_pol / its batch twin: the integrate kernel's hit momenta
    Grow hotspot;   // lt_hotspot_lightcurve: the first stage's partial sums
    Grow spectrum;  // lt_*_spectrum: the first stage's partial histograms of one batch of times (<= LT_SPECTRUM_WORKSPACE_BYTES)
    Grow visibility; // lt_*_visibility: the baselines, then the first stage's partials of one launch (<= LT_VISIBILITY_WORKSPACE_BYTES)
    std::vector<int32_t> blocks_host; // what `blocks` holds (skip the upload when unchanged)
    EventQuad own{}; // lt_render's private timing events (created on first use)
    bool own_ok = false;
    std::vector<EventQuad> aa_events; // lt_render_aa's: one quad per band, grown to the most bands a call had
    Grow aa_list;    // lt_render_aa_adaptive: the count (first 256 bytes) and the list of refined pixels
    Grow aa_scratch; // ... and the base pass's cover / rgb when the caller did not ask for them
    // The tail split of the plain frame path (render_dev_impl): the stream the queue's tail is integrated on and the two
    // events that fork it off `stream` and join it back, all three or none (slot_side, created on first use).
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};

struct Ctx {
    std::vector<StreamSlot *> slots;
    std::vector<EventQuad> pending; // recorded by lt_render_dev(timing=1), not yet collected
    std::vector<EventQuad> pool;
};

// lt_render's private timing events of a slot, all four or none (a failed creation leaves nothing behind)
static int slot_events(StreamSlot *sl)
{
    if (sl->own_ok) return LT_OK;
    int made = 0;
    for (auto &e : sl->own.e) {
        if (hipEventCreate(&e) != hipSuccess) break;
        ++made;
    }
    if (made != (int)(sizeof(sl->own.e) / sizeof(sl->own.e[0]))) {
        for (int j = 0; j < made; ++j) (void)hipEventDestroy(sl->own.e[j]);
        return fail(LT_ERR_HIP, "hipEventCreate failed");
    }
    sl->own_ok = true;
    return LT_OK;
}

// The side stream of a slot and its fork / join events, all three or none.  Non-blocking (it is ordered against `stream`
// by the two events alone, also when `stream` is the legacy default stream) and of the lowest priority the device has:
// the work put there is meant to take the wave slots the user's stream leaves free, not to compete for them.
static int slot_side(StreamSlot *sl)
{
    if (sl->side) return LT_OK;
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    hipError_t e = hipStreamCreateWithPriority(&side, hipStreamNonBlocking, least);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&join, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (join) (void)hipEventDestroy(join);
        if (fork) (void)hipEventDestroy(fork);
        if (side) (void)hipStreamDestroy(side);
        return fail(LT_ERR_HIP, "creating the side stream of a slot failed: %s", hipGetErrorString(e));
    }
    sl->side = side; sl->fork = fork; sl->join = join;
    return LT_OK;
}

static std::mutex g_mu;
static Ctx g_ctx[64];
struct MultiStream { int dev, idx; hipStream_t s; }; // lt_render_multi: one stream per (device, partition)
static std::vector<MultiStream> g_multi_streams;

static int cur_ctx(Ctx **out)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(LT_ERR_INVALID_ARG, "device index %d out of range", dev);
    *out = &g_ctx[dev];
    return LT_OK;
}

static int get_slot(hipStream_t s, StreamSlot **out)
{
    Ctx *c;
    int rc = cur_ctx(&c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    for (StreamSlot *sl : c->slots)
        if (sl->stream == s) { *out = sl; return LT_OK; }
    StreamSlot *sl = new StreamSlot;
    sl->stream = s;
    c->slots.push_back(sl);
    *out = sl;
    return LT_OK;
}

// Draining `stream` is enough before the buffer is replaced.  Every launch that touches it is on `stream`, with one
// exception: the tail split of render_dev_impl integrates the end of the tile queue on the slot's side stream.  That
// call makes `stream` wait for the side stream's join event before it returns (SideJoin, on its error returns too), so
// whatever the side stream was given completes before anything enqueued on `stream` afterwards -- this drain included.
static int grow(Grow &g, size_t need, hipStream_t stream)
{
    if (need <= g.bytes) return LT_OK;
    if (g.p) {
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipFree(g.p));
        g.p = nullptr;
        g.bytes = 0;
    }
    need = (need + 4095) & ~(size_t)4095;
    HIP_TRY(hipMalloc(&g.p, need));
    g.bytes = need;
    return LT_OK;
}

static void release(Grow &g)
{
    if (g.p) (void)hipFree(g.p);
    g.p = nullptr;
    g.bytes = 0;
}

// Everything a slot owns, and the slot.  The caller has drained the slot's stream and taken the slot off its list.
static void destroy_slot(StreamSlot *sl)
{
    for (Grow *g : {&sl->ws, &sl->dev, &sl->dense, &sl->blocks, &sl->disk_img, &sl->disk_time, &sl->disk_mom, &sl->hotspot, &sl->spectrum, &sl->visibility, &sl->aa_list, &sl->aa_scratch}) release(*g);
    if (sl->own_ok) for (auto &e : sl->own.e) (void)hipEventDestroy(e);
    for (auto &q : sl->aa_events) for (auto &e : q.e) (void)hipEventDestroy(e);
    if (sl->side) { // (joined into the slot's stream by every call that used it; drained here all the same)
        (void)hipStreamSynchronize(sl->side);
        (void)hipEventDestroy(sl->fork);
        (void)hipEventDestroy(sl->join);
        (void)hipStreamDestroy(sl->side);
    }
    delete sl;
}

// Workspace layout: 256 B of control words (queue head; at byte 128 the head of the tail split's second part) | STAT_SLOTS x 8 partial counters of the epilogue | ic[n_q] |
// fin0[n_q] | fin1[n_q], each a 4-vector of T.  The partial counters are zero between frames (zeroed when the buffer
// is allocated, and again by k_stats_reduce after it has read them).
constexpr size_t WS_CTRL_BYTES = 256 + (size_t)STAT_SLOTS * 8 * sizeof(unsigned long long);
struct Workspace {
    unsigned long long *head, *head_b, *partials;
    char *records; // ic, fin0, fin1: n_q records each, of the precision the workspace was asked for
    size_t n_q;
    template <typename T> typename Vec4<T>::type *ic() const { return (typename Vec4<T>::type *)records; }
    template <typename T> typename Vec4<T>::type *fin0() const { return ic<T>() + n_q; }
    template <typename T> typename Vec4<T>::type *fin1() const { return ic<T>() + 2 * n_q; }
};

// The one place a precision (32 or 64, check_opts) becomes a type: f(T{}) with T = float or double.
template <typename F> static auto with_precision(int precision, F f) { return precision == 32 ? f(float{}) : f(double{}); }
static size_t elem_size(int precision) { return precision == 32 ? sizeof(float) : sizeof(double); }

// Every caller may write records, so the slot's record key (IcKey) is cleared here; the frame path asks for the key the
// slot held (`held`; invalid when the buffer was replaced) and sets it again itself.
static int get_workspace(hipStream_t stream, size_t n_q, size_t elem, Workspace *w, StreamSlot **slot = nullptr,
                         IcKey *held = nullptr)
{
    StreamSlot *sl;
    int rc = get_slot(stream, &sl);
    if (rc) return rc;
    if (slot) *slot = sl;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (held) *held = sl->ic_key;
        sl->ic_key.valid = false;
    }
    size_t vec = 4 * elem;
    const void *before = sl->ws.p;
    const size_t bytes_before = sl->ws.bytes;
    if ((rc = grow(sl->ws, WS_CTRL_BYTES + 3 * n_q * vec, stream))) return rc;
    if (held && sl->ws.bytes != bytes_before) held->valid = false; // (a replaced buffer may come back at the same address)
    if (sl->ws.p != before) HIP_TRY(hipMemsetAsync(sl->ws.p, 0, WS_CTRL_BYTES, stream)); // a new buffer: control words and partial counters start at zero
    char *base = (char *)sl->ws.p;
    w->head = (unsigned long long *)base;
    w->head_b = (unsigned long long *)(base + 128);
    w->partials = (unsigned long long *)(base + 256);
    w->records = base + WS_CTRL_BYTES;
    w->n_q = n_q;
    return LT_OK;
}

// Carves 256-byte aligned pieces out of one grow-only buffer.
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};

static int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

// LT_IC_REUSE=0: k_prologue_camera runs every frame, as if no key ever matched (A/B measurements, bisecting).
static bool ic_reuse_enabled()
{
    static const bool on = env_int("LT_IC_REUSE", 1) != 0;
    return on;
}

// LT_EQ_STREAK=0 / lt_set_eq_streak(0): the float32 streak's fixed-quadrant loop is never entered (its band is empty), as
// before it existed (A/B measurements, bisecting, tests/test_gpu_eq_streak.py).  Read by make_kerr for every launch.
static std::atomic<int> g_eq_streak{-1}; // -1: not yet read from the environment
static bool eq_streak_enabled()
{
    int v = g_eq_streak.load(std::memory_order_relaxed);
    if (v < 0) {
        v = env_int("LT_EQ_STREAK", 1) != 0;
        int unset = -1;
        if (!g_eq_streak.compare_exchange_strong(unset, v)) v = unset;
    }
    return v != 0;
}
extern "C" int lt_set_eq_streak(int on)
{
    const int before = eq_streak_enabled();
    g_eq_streak.store(on != 0);
    return before;
}

// LT_UNIT_STREAK=0 / lt_set_unit_streak(0): the fixed-quadrant loop never takes its unit-step form (A/B measurements,
// bisecting, tests/test_gpu_unit_streak.py).  Read by make_kerr for every launch.
static std::atomic<int> g_unit_streak{-1}; // -1: not yet read from the environment
static bool unit_streak_enabled()
{
    int v = g_unit_streak.load(std::memory_order_relaxed);
    if (v < 0) {
        v = env_int("LT_UNIT_STREAK", 1) != 0;
        int unset = -1;
        if (!g_unit_streak.compare_exchange_strong(unset, v)) v = unset;
    }
    return v != 0;
}
extern "C" int lt_set_unit_streak(int on)
{
    const int before = unit_streak_enabled();
    g_unit_streak.store(on != 0);
    return before;
}

// The tail split of the plain frame path (render_dev_impl): the last tile rows of the queue are integrated
// by a launch of their own on the slot's side stream.  LT_TAIL_SPLIT / lt_set_tail_split(n): -1 the automatic size,
// 0 off, n > 0 that many tile rows, clamped to what the frame allows.  Read by render_dev_impl for every frame.
constexpr int TAIL_SPLIT_DEFAULT = -1; // (automatic: profiles/tail_split_ab.txt)
static std::atomic<int> g_tail_split{INT32_MIN}; // INT32_MIN: not yet read from the environment
static int tail_split_request()
{
    int v = g_tail_split.load(std::memory_order_relaxed);
    if (v == INT32_MIN) {
        v = env_int("LT_TAIL_SPLIT", TAIL_SPLIT_DEFAULT);
        if (v < -1) v = -1;
        int unset = INT32_MIN;
        if (!g_tail_split.compare_exchange_strong(unset, v)) v = unset;
    }
    return v;
}
extern "C" int lt_set_tail_split(int tile_rows)
{
    const int before = tail_split_request();
    g_tail_split.store(tile_rows < -1 ? -1 : tile_rows);
    return before;
}

// Where the tail split cuts a frame's tile queue (queue_pos_to_tile, lt_kernels.hpp): host arithmetic only.  The queue
// ends with the whole tile rows below the hot rectangle, ty >= hot_y1, row-major over the cw = tiles_x - strip width
// columns beside the strip (without a rectangle hot_y1 is 0 and that is every row).  Part B is the last `rows_b` of them,
// queue positions [pos_split, n_tiles) with pos_split = n_tiles - rows_b * cw; part A is everything before, which holds
// every tile with ty < ty_split = tiles_y - rows_b and every tile of the strip.
//   request > 0:  rows_b = request, at most the rows below the rectangle, and part A keeps at least one tile
//   request == -1: rows_b = ceil(TAIL_SPLIT_FILLS * slots / cw), one fill of the chip's `slots` wave slots (measured at
//                  4096^2: half a fill gains a third less, two fills the same -- profiles/tail_split_ab.txt); declines
//                  where that is more than the rows below the rectangle, or where part A would be left with less than
//                  TAIL_SPLIT_MIN_FILLS_A fills (a frame that short is bound by its longest ray, not by the ramp-down)
// Returns false where the frame is not split (then ty_split = tiles_y, pos_split = n_tiles).
constexpr int TAIL_SPLIT_FILLS_NUM = 1, TAIL_SPLIT_FILLS_DEN = 1, TAIL_SPLIT_MIN_FILLS_A = 1;
static bool tail_split_plan(int tiles_x, int tiles_y, int strip_w, int hot_y1, int slots, int request, int *ty_split,
                            int64_t *pos_split)
{
    const int64_t n_tiles = (int64_t)tiles_x * tiles_y;
    *ty_split = tiles_y;
    *pos_split = n_tiles;
    const int64_t cw = (int64_t)tiles_x - strip_w;
    int64_t avail = (int64_t)tiles_y - hot_y1; // tile rows below the rectangle
    if (request == 0 || cw <= 0 || avail <= 0) return false;
    int64_t rows_b;
    if (request > 0) {
        if (avail * cw >= n_tiles) --avail; // (no strip and no rectangle: the first tile row stays in part A)
        rows_b = request < avail ? request : avail;
    } else {
        if (slots <= 0) return false;
        rows_b = ((int64_t)TAIL_SPLIT_FILLS_NUM * slots + TAIL_SPLIT_FILLS_DEN * cw - 1) / (TAIL_SPLIT_FILLS_DEN * cw);
        if (rows_b > avail || n_tiles - rows_b * cw < (int64_t)TAIL_SPLIT_MIN_FILLS_A * slots) return false;
    }
    if (rows_b <= 0) return false;
    *ty_split = (int)(tiles_y - rows_b);
    *pos_split = n_tiles - rows_b * cw;
    return true;
}
// (for tests/test_tail_split_host.py: needs no device)
extern "C" int lt_tail_split_plan(int32_t tiles_x, int32_t tiles_y, int32_t strip_x0, int32_t strip_x1, int32_t hot_y1, int32_t slots,
                                  int32_t request, int32_t *ty_split, int64_t *pos_split)
{
    int ty = 0;
    int64_t pos = 0;
    if (tiles_x <= 0 || tiles_y <= 0 || strip_x0 < 0 || strip_x1 < strip_x0 || strip_x1 > tiles_x || hot_y1 < 0 || hot_y1 > tiles_y) return -1;
    const bool on = tail_split_plan(tiles_x, tiles_y, strip_x1 - strip_x0, hot_y1, slots, request, &ty, &pos);
    if (ty_split) *ty_split = ty;
    if (pos_split) *pos_split = pos;
    return on ? 1 : 0;
}

// Frames of render_dev_impl that were split / that ran as one integrate launch, since the library was loaded.
static uint64_t g_split_frames = 0, g_whole_frames = 0; // (under g_mu)
extern "C" void lt_tail_split_counts(uint64_t *split, uint64_t *whole)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (split) *split = g_split_frames;
    if (whole) *whole = g_whole_frames;
}

// Frames that reused the ray records of their slot / that ran k_prologue_camera, since the library was loaded.
static uint64_t g_ic_hits = 0, g_ic_misses = 0; // (under g_mu)
extern "C" void lt_ic_reuse_counts(uint64_t *hits, uint64_t *misses)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (hits) *hits = g_ic_hits;
    if (misses) *misses = g_ic_misses;
}

static int cu_count(int *out)
{
    static int cached[64];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (!cached[dev & 63]) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        cached[dev & 63] = prop.multiProcessorCount;
    }
    *out = cached[dev & 63];
    return LT_OK;
}

// Frees what the library holds for (current device, stream): call it before destroying a stream that was used
// with the library, or the buffers stay until lt_shutdown().
extern "C" int lt_release_stream(void *stream)
{
    int rc = require_device();
    if (rc) return rc;
    Ctx *c;
    if ((rc = cur_ctx(&c))) return rc;
    StreamSlot *found = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        for (size_t i = 0; i < c->slots.size(); ++i)
            if (c->slots[i]->stream == (hipStream_t)stream) {
                found = c->slots[i];
                c->slots.erase(c->slots.begin() + (long)i);
                break;
            }
    }
    if (!found) return LT_OK;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    destroy_slot(found);
    return LT_OK;
}

extern "C" int lt_shutdown(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    int n = lt_device_count();
    int keep = 0;
    if (n > 0) (void)hipGetDevice(&keep);
    for (int d = 0; d < n && d < 64; ++d) {
        Ctx &c = g_ctx[d];
        if (c.slots.empty() && c.pool.empty() && c.pending.empty()) continue;
        (void)hipSetDevice(d);
        (void)hipDeviceSynchronize();
        for (StreamSlot *sl : c.slots) destroy_slot(sl);
        c.slots.clear();
        for (auto &q : c.pending) for (auto &e : q.e) (void)hipEventDestroy(e);
        for (auto &q : c.pool) for (auto &e : q.e) (void)hipEventDestroy(e);
        c.pending.clear();
        c.pool.clear();
    }
    for (auto &m : g_multi_streams) {
        (void)hipSetDevice(m.dev);
        (void)hipStreamDestroy(m.s);
    }
    g_multi_streams.clear();
    if (n > 0) (void)hipSetDevice(keep);
    return LT_OK;
}

extern "C" void lt_default_opts(lt_opts *o)
{
    memset(o, 0, sizeof(*o));
    o->bg_sampling = LT_BG_GLOBAL; // measured (profiles/r02_background_sampling.txt): the gather itself is 0.06 ms of a 4096^2 frame
    o->integrator = LT_INTEGRATOR_RK4;
    o->precision = 32;
    o->schedule = LT_SCHED_DIRECT;
    o->row_block = 16;
    o->n_parts = 1;
    o->axis_refine_frac = 0.07;
    o->phi_max = 50.0;
    o->h_max = 0.0; // 0 -> metric default (0.05 Schwarzschild, 1.0 Kerr)
}

// ---------------------------------------------------------------------------------------------
// constant blocks
// ---------------------------------------------------------------------------------------------
// _psi_frame, image_lens.py:21-61.
static void psi_frame(double psi_y, double psi_x, double *d, double *ex, double *ey, bool *in_front)
{
    d[0] = sin(psi_x) * cos(psi_y);
    d[1] = -sin(psi_y);
    d[2] = cos(psi_x) * cos(psi_y);
    *in_front = d[2] > 1e-12;
    auto dot = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    auto norm = [&](const double *a) { return sqrt(dot(a, a)); };
    const double cx[3] = {1, 0, 0}, cy[3] = {0, 1, 0};
    double t = dot(cx, d);
    for (int i = 0; i < 3; ++i) ex[i] = cx[i] - t * d[i];
    double n = norm(ex);
    if (n < 1e-12) {
        t = dot(cy, d);
        for (int i = 0; i < 3; ++i) ex[i] = cy[i] - t * d[i];
        n = norm(ex);
    }
    n = n > 1e-12 ? n : 1e-12;
    for (int i = 0; i < 3; ++i) ex[i] /= n;
    double t1 = dot(cy, d), t2 = dot(cy, ex);
    for (int i = 0; i < 3; ++i) ey[i] = cy[i] - t1 * d[i] - t2 * ex[i];
    n = norm(ey);
    if (n < 1e-12) {
        ey[0] = d[1] * ex[2] - d[2] * ex[1];
        ey[1] = d[2] * ex[0] - d[0] * ex[2];
        ey[2] = d[0] * ex[1] - d[1] * ex[0];
        n = norm(ey);
    }
    n = n > 1e-12 ? n : 1e-12;
    for (int i = 0; i < 3; ++i) ey[i] /= n;
}

extern "C" int64_t lt_local_rows(int32_t height, int32_t row_block, int32_t n_parts, int32_t part)
{
    if (height <= 0 || row_block <= 0 || n_parts <= 0 || part < 0 || part >= n_parts) return -1;
    int64_t rows = 0;
    for (int64_t b = part; b * row_block < height; b += n_parts) {
        int64_t r0 = b * row_block, r1 = r0 + row_block;
        rows += (r1 < height ? r1 : height) - r0;
    }
    return rows;
}

extern "C" int64_t lt_global_row(int64_t local_row, int32_t row_block, int32_t n_parts, int32_t part)
{
    int64_t b = local_row / row_block, o = local_row - b * row_block;
    return (b * n_parts + part) * row_block + o;
}

// Row blocks partition `o.part` owns (ascending) and how many rows that is.  Block-cyclic unless a table is given.
static int partition_blocks(int32_t height, const lt_opts &o, std::vector<int32_t> *blocks, int64_t *rows)
{
    const int64_t nb = (height + (int64_t)o.row_block - 1) / o.row_block;
    if (o.block_owner && o.n_blocks != nb)
        return fail(LT_ERR_INVALID_ARG, "block_owner has %d entries, the frame has %lld row blocks of %d rows", o.n_blocks,
                    (long long)nb, o.row_block);
    *rows = 0;
    if (blocks) blocks->clear();
    for (int64_t b = 0; b < nb; ++b) {
        int owner = o.block_owner ? (int)o.block_owner[b] : (int)(b % o.n_parts);
        if (o.block_owner && owner >= o.n_parts) return fail(LT_ERR_INVALID_ARG, "block_owner[%lld] = %d, n_parts = %d", (long long)b, owner, o.n_parts);
        if (owner != o.part) continue;
        int64_t r0 = b * o.row_block, r1 = r0 + o.row_block;
        *rows += (r1 < height ? r1 : height) - r0;
        if (blocks) blocks->push_back((int32_t)b);
    }
    return LT_OK;
}

static int make_metric(const lt_metric *m, double r_obs, double theta_obs, double h_schw, MetricConsts *mc)
{
    if (!(m->M > 0.0)) return fail(LT_ERR_INVALID_ARG, "M must be positive");
    mc->kind = m->kind;
    mc->M = m->M;
    mc->a = m->kind == LT_METRIC_KERR ? m->a : 0.0;
    if (m->kind == LT_METRIC_KERR && fabs(m->a) > m->M)
        return fail(LT_ERR_INVALID_ARG, "|a|=%g exceeds M=%g", fabs(m->a), m->M); // metrics.py:849-850
    if (m->kind != LT_METRIC_KERR && m->kind != LT_METRIC_SCHWARZSCHILD)
        return fail(LT_ERR_INVALID_ARG, "unknown metric kind %d", m->kind);
    mc->r_obs = r_obs;
    mc->theta_obs = theta_obs;
    mc->r_plus = mc->M + sqrt(mc->M * mc->M - mc->a * mc->a); // metrics.py:853
    mc->r_capture = mc->r_plus * 1.01;                        // metrics.py:428, :579
    mc->R_S = 2.0 * mc->M;                                    // metrics.py:742
    mc->phi_h = h_schw;
    mc->evals_fixed = 0;
    mc->evals_per_step = 4;
    { // the observer-only part of metrics.py:148-218, in its operation order (K1 used to redo this per ray)
        double r = r_obs, a = mc->a, M_ = mc->M;
        double sin_th = sin(theta_obs), cos_th = cos(theta_obs);
        double sin_th_sq = sin_th * sin_th;
        if (sin_th_sq < 1e-15) sin_th_sq = 1e-15;
        double Sigma = r * r + a * a * cos_th * cos_th;
        double Delta = r * r - 2.0 * M_ * r + a * a;
        mc->obs_ok = Delta > 0.0 && Sigma > 0.0;
        mc->obs_sin_th = sin_th; mc->obs_cos2 = cos_th * cos_th; mc->obs_sin2 = sin_th_sq;
        mc->obs_sqrt_Sigma = mc->obs_ok ? sqrt(Sigma) : 0.0;
        mc->obs_sqrt_Delta = mc->obs_ok ? sqrt(Delta) : 1.0;
        double A_val = (r * r + a * a) * (r * r + a * a) - a * a * Delta * sin_th_sq;
        double SD = mc->obs_ok ? Sigma * Delta : 1.0;
        mc->obs_g_tt = -A_val / SD;
        mc->obs_g_tphi = -2.0 * M_ * a * r / SD;
        mc->obs_g_rr = mc->obs_ok ? Delta / Sigma : 1.0;
        mc->obs_g_thth = mc->obs_ok ? 1.0 / Sigma : 0.0;
        mc->obs_g_phiphi = (Delta - a * a * sin_th_sq) / (SD * sin_th_sq);
    }
    return LT_OK;
}

template <typename T> static KerrConsts<T> make_kerr(const MetricConsts &mc, double lambda_max, double h_max)
{
    KerrConsts<T> k;
    k.M = (T)mc.M; k.a = (T)mc.a; k.a2 = (T)(mc.a * mc.a); k.two_M = (T)(2.0 * mc.M);
    k.r_cut = (T)(mc.r_plus * 1.001);
    k.r_capture = (T)mc.r_capture;
    k.r_escape = (T)(mc.r_obs * 2.0);
    k.r_obs = (T)mc.r_obs; k.theta_obs = (T)mc.theta_obs;
    k.lambda_max = (T)lambda_max;
    k.h_max = (T)h_max;
    k.rc4 = (T)(mc.r_capture * 4.0); k.rc2 = (T)(mc.r_capture * 2.0); k.rc12 = (T)(mc.r_capture * 1.2);
    // the fixed-quadrant band of the float32 streak; empty (no angle is inside) with the switch off and for float64
    const bool eq = sizeof(T) == 4 && eq_streak_enabled();
    k.eq_lo = eq ? (T)M<float>::EQ_BAND_LO : (T)1;
    k.eq_hi = eq ? (T)M<float>::EQ_BAND_HI : (T)0;
    // the unit-step form of that loop: the loop's own range limit lambda_max - h_base at h_base = 1, in the kernel's
    // arithmetic; never taken with the switch off or beyond the range its margin is proved for (kerr_rk4_streak)
    const bool unit = eq && unit_streak_enabled() && k.lambda_max <= (T)8192;
    k.unit_lam = unit ? (T)(k.lambda_max - (T)1) : -(T)INFINITY;
    return k;
}

// The steps of the reference's loop (metrics.py:68-73): while phi < phi_max, h = min(h_max, phi_max - phi), phi += h, with
// phi ACCUMULATED in float64.  The sum of n_full steps seldom lands on phi_max exactly, so a range that is a whole multiple
// of h_max on paper (50 / 0.05) still ends in a step of the rounding's size (7e-13), four evaluations that a closed form
// floor(phi_max / h_max) leaves out.  The loop is run here once per launch, in float64 whatever the kernel's precision
// (the fixtures are the float64 reference's): n_full full steps, then h_last > 0 if a shorter one follows.  The shorter
// step ends the range: remaining < h_max <= phi puts phi within a factor two of phi_max, where phi_max - phi and
// phi + (phi_max - phi) are both exact.
// (check_opts refuses a range of more than SCHW_MAX_STEPS steps: the loop below is bounded by it, and phi += h_max always
// moves phi -- h_max >= phi_max / 2^24 is far above an ulp of any phi <= phi_max.)
constexpr uint32_t SCHW_MAX_STEPS = 1u << 24;
static void schw_step_plan(double phi_max, double h_max, uint32_t *n_full, double *h_last)
{
    double phi = 0.0;
    uint32_t nf = 0;
    *h_last = 0.0;
    while (phi < phi_max && nf <= SCHW_MAX_STEPS) {
        double h = h_max, remaining = phi_max - phi;
        if (remaining < h) h = remaining;
        if (h <= 0.0) break;
        if (h < h_max) { *h_last = h; break; }
        phi += h;
        ++nf;
    }
    *n_full = nf;
}

template <typename T> static SchwConsts<T> make_schw(const MetricConsts &mc, double phi_max, double h_max)
{
    SchwConsts<T> k;
    double rest;
    k.M = (T)mc.M; k.three_M = (T)(3.0 * mc.M);
    k.u0 = (T)(1.0 / mc.r_obs);
    k.u_capture = (T)(1.0 / (mc.R_S * 1.01)); // metrics.py:66
    k.u_escape = (T)(1.0 / (2.0 * mc.r_obs)); // metrics.py:67
    k.h_max = (T)h_max; k.phi_max = (T)phi_max;
    schw_step_plan(phi_max, h_max, &k.n_full, &rest);
    k.h_last = (T)rest;
    return k;
}

// ---------------------------------------------------------------------------------------------
// stage launchers
// ---------------------------------------------------------------------------------------------
// Brackets the three kernels of one frame with HIP events.  Two modes: a quad from the device's pool that
// ends up on the `pending` list for lt_timing_collect (lt_render_dev with opts->timing), or a caller-owned
// quad (lt_render's private one, read directly).  A quad taken from the pool goes back to it on every
// path that does not finish().
struct Timer {
    bool on = false, pooled = false, done = false;
    EventQuad q{};
    Ctx *ctx = nullptr;
    ~Timer()
    {
        if (on && pooled && !done) {
            std::lock_guard<std::mutex> lk(g_mu);
            ctx->pool.push_back(q);
        }
    }
    int begin(bool enable, const EventQuad *own)
    {
        if (own) { on = true; q = *own; return LT_OK; }
        if (!enable) return LT_OK;
        int rc = cur_ctx(&ctx);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(g_mu);
        if (!ctx->pool.empty()) { q = ctx->pool.back(); ctx->pool.pop_back(); }
        else {
            for (int i = 0; i < 4; ++i) {
                hipError_t e = hipEventCreate(&q.e[i]);
                if (e != hipSuccess) {
                    for (int j = 0; j < i; ++j) (void)hipEventDestroy(q.e[j]);
                    return fail(LT_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e));
                }
            }
        }
        on = pooled = true;
        return LT_OK;
    }
    int mark(int i, hipStream_t s)
    {
        if (on) HIP_TRY(hipEventRecord(q.e[i], s));
        return LT_OK;
    }
    void finish()
    {
        if (!on || !pooled) return;
        std::lock_guard<std::mutex> lk(g_mu);
        ctx->pending.push_back(q);
        done = true;
    }
};

extern "C" int lt_timing_collect(double *prologue_ms, double *integrate_ms, double *epilogue_ms, int32_t *calls)
{
    Ctx *c;
    int rc = cur_ctx(&c);
    if (rc) return rc;
    double t[3] = {0, 0, 0};
    std::lock_guard<std::mutex> lk(g_mu);
    int n = 0;
    for (auto &q : c->pending) {
        HIP_TRY(hipEventSynchronize(q.e[3]));
        for (int i = 0; i < 3; ++i) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, q.e[i], q.e[i + 1]));
            t[i] += ms;
        }
        c->pool.push_back(q);
        ++n;
    }
    c->pending.clear();
    if (prologue_ms) *prologue_ms = t[0];
    if (integrate_ms) *integrate_ms = t[1];
    if (epilogue_ms) *epilogue_ms = t[2];
    if (calls) *calls = n;
    return LT_OK;
}

// Diagnostic wave stamps (LT_STAMPS_FILE=path): one uint4 per wavefront, dumped raw after the launch.
struct StampDump {
    const char *path = getenv("LT_STAMPS_FILE");
    uint4 *dev = nullptr;
    size_t n = 0;
    int begin(size_t waves)
    {
        if (!path) return LT_OK;
        n = waves;
        HIP_TRY(hipMalloc((void **)&dev, n * sizeof(uint4)));
        HIP_TRY(hipMemset(dev, 0, n * sizeof(uint4)));
        return LT_OK;
    }
    int end()
    {
        if (!path) return LT_OK;
        std::vector<uint4> h(n);
        HIP_TRY(hipMemcpy(h.data(), dev, n * sizeof(uint4), hipMemcpyDeviceToHost));
        HIP_TRY(hipFree(dev));
        if (FILE *f = fopen(path, "wb")) { fwrite(h.data(), sizeof(uint4), n, f); fclose(f); }
        return LT_OK;
    }
};

// Wavefront slots of the device for a kernel launched with 64-thread workgroups (0 if the query fails: the caller then
// launches one workgroup per tile).  Asked once per kernel.
template <auto Kernel> static int resident_slots()
{
    static const int slots = [] {
        int per_cu = 0, cus = 0;
        if (cu_count(&cus) != LT_OK) return 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)Kernel, 64, 0) != hipSuccess || per_cu <= 0) return 0;
        return per_cu * cus;
    }();
    return slots;
}

// The kernels of the direct schedule, by integrator: the plain frame path and the two disks (lt_disk.hpp, lt_disk_images.hpp).
template <typename T> struct PlainKernels { template <typename Integ> static constexpr auto kernel = &k_kerr_direct<T, Integ>; };
template <typename T> struct DiskKernels { template <typename Integ> static constexpr auto kernel = &k_kerr_disk<T, Integ>; };
template <typename T> struct DiskImagesKernels { template <typename Integ> static constexpr auto kernel = &k_kerr_disk_images<T, Integ>; };
template <typename T> struct DiskTimedKernels { template <typename Integ> static constexpr auto kernel = &k_kerr_disk_timed<T, Integ>; };
template <typename T> struct DiskPolKernels { template <typename Integ> static constexpr auto kernel = &k_kerr_disk_pol<T, Integ>; };
template <typename Integ> struct IntegTag { using type = Integ; };

// The switches of the direct schedule, read once.
struct DirectTuning {
    // LT_D_LONG: steps after which a wavefront is "long" (ghost lanes, lone-wave step form, issue priority).  384: with the
    // packed lone-wave step of round 2 an earlier switch pays on chain-bound launches -- 2048^2 4.19 -> 4.10 ms, one rank
    // of 8 4.00 -> 3.95, of 4 4.18 -> 4.12 -- and leaves the 4096^2 frame where it was (10.75 / 10.73 ms); 128 costs that
    // frame 1.5 % (profiles/r03_xcd_clock.txt, tools/scratch/d_long_sweep.sh)
    int long_iters;
    // LT_D_PERSIST: tiles are handed out from a queue head to a grid that fills the chip once (direct_tiles); 0, or wider
    // workgroups: one workgroup per tile, as in round 1.
    int persist;
};
static const DirectTuning &direct_tuning()
{
    static const DirectTuning t{env_int("LT_D_LONG", 384), env_int("LT_D_PERSIST", 1)};
    return t;
}

// The integrator of a Kerr launch as a type, for both schedules: go(IntegTag<Integ>{}, long_steps).  `long_rk4`: step
// attempts after which a wavefront counts as long, for RK4 -- DP45 rays take ~50 attempts, not ~150, so a third of it.
template <typename T, typename Go> static int with_integrator(const lt_opts &o, int long_rk4, Go go)
{
    const bool exact = o.integrator == LT_INTEGRATOR_DP45_EXACT;
    const bool dp45 = o.integrator == LT_INTEGRATOR_DP45 || exact;
    if (dp45 && sizeof(T) != 8) return fail(LT_ERR_UNSUPPORTED, "DP45 needs precision 64");
    if constexpr (sizeof(T) == 8) {
        if (exact) return go(IntegTag<Dp45<T, true>>{}, long_rk4 / 3);
        if (dp45) return go(IntegTag<Dp45<T>>{}, long_rk4 / 3);
    }
    return go(IntegTag<Rk4<T>>{}, long_rk4);
}

// A run of queue positions of the direct schedule and the head word its launch hands them out from: the whole queue, or
// one of the two parts the tail split cuts it into (render_dev_impl).
struct QueuePart {
    int64_t tile0, n_tiles;
    unsigned long long *head;
    int64_t q_end() const { return (tile0 + n_tiles) * 64; } // what the kernel's end test compares with
};

// One launch of the direct schedule (direct_tiles, lt_kernels.hpp) over the queue part `part`: picks the integrator's
// kernel of the family `Kernels`, sizes the grid to the part -- one wavefront per resident slot and the part's head word,
// or one workgroup per tile and no head when the part fits the chip --, zeroes the head and calls
// launch(kernel, grid, long_iters, head), which adds the family's own arguments.  `block`: work-items per workgroup (64
// everywhere but under LT_K2_BLOCK on the plain frame path).
template <typename T, typename Kernels, typename Launch>
static int launch_direct(const lt_opts &o, const QueuePart &part, hipStream_t s, int block, Launch launch)
{
    const DirectTuning &tune = direct_tuning();
    return with_integrator<T>(o, tune.long_iters, [&](auto integ, int long_it) -> int {
        constexpr auto kernel = Kernels::template kernel<typename decltype(integ)::type>;
        unsigned grid = (unsigned)((part.n_tiles * 64 + block - 1) / block);
        unsigned long long *head = nullptr;
        const int slots = tune.persist && block == 64 ? resident_slots<kernel>() : 0;
        if (slots > 0 && (unsigned)slots < grid) { grid = (unsigned)slots; head = part.head; } // (a launch that fits the chip needs no queue)
        if (head) HIP_TRY(hipMemsetAsync(head, 0, sizeof(unsigned long long), s));
        launch(kernel, grid, (uint32_t)long_it, head);
        HIP_TRY(hipGetLastError());
        return LT_OK;
    });
}
// ... over the whole queue (the disks)
template <typename T, typename Kernels, typename Launch>
static int launch_direct(const lt_opts &o, const Workspace &w, int64_t n_q, hipStream_t s, int block, Launch launch)
{
    return launch_direct<T, Kernels>(o, QueuePart{0, n_q / 64, w.head}, s, block, launch);
}

// Work-items per workgroup of the plain frame path's direct kernel (LT_K2_BLOCK: 64, 128 or 256).
static int k2_block()
{
    static const int b = [] { int v = env_int("LT_K2_BLOCK", 64); return (v == 64 || v == 128 || v == 256) ? v : 64; }();
    return b;
}

// Wavefront slots the plain frame path's direct kernel of these options fills the chip with (0: it does not run as a
// persistent grid -- LT_D_PERSIST=0, wider workgroups, or the occupancy query failed).
template <typename T> static int direct_slots(const lt_opts &o)
{
    int slots = 0;
    if (!direct_tuning().persist || k2_block() != 64) return 0;
    (void)with_integrator<T>(o, 0, [&](auto integ, int) -> int {
        slots = resident_slots<PlainKernels<T>::template kernel<typename decltype(integ)::type>>();
        return LT_OK;
    });
    return slots;
}

template <typename T>
static int launch_integrate(const MetricConsts &mc, const lt_opts &o, double lambda_max, const Workspace &w,
                            int64_t n_q, hipStream_t s, uint64_t *kstats, const QueuePart *part = nullptr)
{
    int rc;
    unsigned grid = (unsigned)((n_q + 255) / 256);
    if (mc.kind == LT_METRIC_SCHWARZSCHILD) {
        SchwConsts<T> k = make_schw<T>(mc, o.phi_max, o.h_max);
        k_schw_rk4_direct<T><<<grid, 256, 0, s>>>(k, w.ic<T>(), w.fin0<T>(), w.fin1<T>(), n_q);
    } else {
        KerrConsts<T> k = make_kerr<T>(mc, lambda_max, o.h_max);
        StampDump sd;
        if (o.schedule == LT_SCHED_DIRECT) {
            // wider workgroups and the per-wave stamps (StampDump) exist on this path only, not for the disks
            // `part`: the queue positions of this launch (the tail split); NULL: the whole queue
            const QueuePart qp = part ? *part : QueuePart{0, n_q / 64, w.head};
            if ((rc = sd.begin((size_t)(n_q / 64)))) return rc;
            rc = launch_direct<T, PlainKernels<T>>(o, qp, s, k2_block(), [&](auto kernel, unsigned kgrid, uint32_t long_iters, unsigned long long *head) {
                kernel<<<kgrid, k2_block(), 0, s>>>(k, w.ic<T>(), w.fin0<T>(), w.fin1<T>(), qp.q_end(), long_iters, sd.dev, kstats, head, qp.tile0);
            });
            if (rc) return rc;
        } else {
            int cus;
            if ((rc = cu_count(&cus))) return rc;
            // persistent grid: blocks-per-CU x CUs, never more blocks than there are 256-ray pieces
            static const int bpc = env_int("LT_Q_BPC", sizeof(T) == 4 ? 8 : 3);
            static const int chunk = env_int("LT_Q_CHUNK", 64);
            static const int refill_min = env_int("LT_Q_REFILL", 4);
            static const int long_steps = env_int("LT_Q_LONG", 600);
            unsigned qgrid = (unsigned)(cus * bpc);
            if (qgrid > grid) qgrid = grid;
            rc = with_integrator<T>(o, long_steps, [&](auto integ, int long_it) -> int {
                HIP_TRY(hipMemsetAsync(w.head, 0, sizeof(unsigned long long), s));
                if (int brc = sd.begin((size_t)qgrid * 4)) return brc;
                k_kerr_queue<T, typename decltype(integ)::type><<<qgrid, 256, 0, s>>>(k, w.ic<T>(), w.fin0<T>(), w.fin1<T>(), (uint64_t)n_q, w.head,
                                                                                     (uint32_t)chunk, (uint32_t)refill_min, (uint32_t)long_it,
                                                                                     sd.dev, kstats);
                return LT_OK;
            });
            if (rc) return rc;
        }
        HIP_TRY(hipGetLastError());
        if ((rc = sd.end())) return rc;
    }
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

static int check_opts(const lt_metric *metric, lt_opts *o)
{
    if (o->precision != 32 && o->precision != 64) return fail(LT_ERR_INVALID_ARG, "precision must be 32 or 64");
    if (metric->kind == LT_METRIC_KERR && (o->integrator == LT_INTEGRATOR_DP45 || o->integrator == LT_INTEGRATOR_DP45_EXACT) &&
        o->precision != 64)
        return fail(LT_ERR_UNSUPPORTED,
                    "DP45 at the reference tolerances needs float64 (rtol 1e-8 is below float32 epsilon)");
    if (o->integrator != LT_INTEGRATOR_DP45 && o->integrator != LT_INTEGRATOR_RK4 && o->integrator != LT_INTEGRATOR_DP45_EXACT)
        return fail(LT_ERR_INVALID_ARG, "unknown integrator %d", o->integrator);
    if (o->schedule != LT_SCHED_DIRECT && o->schedule != LT_SCHED_QUEUE)
        return fail(LT_ERR_INVALID_ARG, "unknown schedule %d", o->schedule);
    if (o->bg_sampling != LT_BG_LDS_TILES && o->bg_sampling != LT_BG_GLOBAL)
        return fail(LT_ERR_INVALID_ARG, "unknown bg_sampling %d", o->bg_sampling);
    if (o->h_max <= 0.0) o->h_max = metric->kind == LT_METRIC_KERR ? 1.0 : 0.05;
    if (o->phi_max <= 0.0) o->phi_max = 50.0;
    if (metric->kind == LT_METRIC_SCHWARZSCHILD && !(o->phi_max / o->h_max <= (double)SCHW_MAX_STEPS))
        return fail(LT_ERR_INVALID_ARG, "phi_max / h_max = %g: more than %u steps per ray", o->phi_max / o->h_max, SCHW_MAX_STEPS);
    if (o->row_block <= 0) o->row_block = 16;
    if (o->n_parts <= 0) o->n_parts = 1;
    if (o->part < 0 || o->part >= o->n_parts) return fail(LT_ERR_INVALID_ARG, "part %d not in [0, %d)", o->part, o->n_parts);
    if (o->block_owner && o->n_blocks <= 0) return fail(LT_ERR_INVALID_ARG, "block_owner given with n_blocks = %d", o->n_blocks);
    return LT_OK;
}

// Observer-frame evaluation counts of the adaptive integrators (make_metric leaves RK4's four per step).
static void count_evals(int integrator, MetricConsts *mc)
{
    if (mc->kind == LT_METRIC_KERR && integrator != LT_INTEGRATOR_RK4) { mc->evals_fixed = 1; mc->evals_per_step = 6; }
}

// The thin disk of lt_render_disk (lt_api_disk.inc): resolved parameters and the extra output.  max_images > 0: the
// optically thin disk of lt_render_disk_images (lt_api_disk_images.inc) and its outputs.
struct DiskParams {
    double r_in, r_out, q, exposure; // r_in resolved (the ISCO when the caller asked for it)
    float *d_disk;                   // (R, W, 3) float32 or NULL
    int max_images = 0;              // slots kept per ray; 0: the opaque disk
    float *d_images = nullptr;       // (R, W, max_images, 3) float32 or NULL
    uint8_t *d_n_hits = nullptr;     // (R, W) or NULL
    bool timed = false;              // lt_trace_disk_hits (lt_api_hotspot.inc): d_images is (R, W, max_images, 4), no colour
    int image_words() const { return timed ? 4 : 3; }
    bool pol = false;                // lt_trace_disk_pol (lt_api_polarization.inc): the timed trace plus d_pol
    PolConsts pc{};                  // ... its observer and field
    void *d_pol = nullptr;           // (R, W, max_images, 4) float32, or (n, max_images, 4) float64 in a batch, or NULL
};
// The hit records of the thin disk, resolved once per call (get_disk_records) and handed to its launches.
struct DiskRecordsBuf {
    void *p = nullptr;        // Vec2<T> [max_images][n_q]
    uint32_t *hits = nullptr; // [n_q]
    void *tim = nullptr;      // the timed trace: T [max_images][n_q]
    void *mom = nullptr;      // the polarized trace: Vec2<T> [max_images][n_q]
    template <typename T> typename Vec2<T>::type *img() const { return (typename Vec2<T>::type *)p; }
};
// The disks' launches, defined in lt_api_disk.inc and lt_api_disk_images.inc (which in turn call the frame plumbing below).
static int get_disk_records(hipStream_t s, int64_t n_q, size_t elem, const DiskParams *disk, DiskRecordsBuf *recs);
template <typename T>
static int launch_integrate_disk(const MetricConsts &mc, const lt_opts &o, double lambda_max, const Workspace &w, int64_t n_q,
                                 hipStream_t s, uint64_t *kstats, const DiskParams &dp, const DiskRecordsBuf &recs);
static int launch_epilogue_disk(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w,
                                const FrameOut &fo, uint64_t *d_stats, hipStream_t s, const DiskParams &dp);
static int launch_epilogue_disk_images(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w,
                                       const FrameOut &fo, uint64_t *d_stats, hipStream_t s, const DiskParams &dp,
                                       const DiskRecordsBuf &recs);
static int launch_epilogue_arrays_disk_images(const MetricConsts &mc, const lt_opts &o, const Workspace &w, int64_t n,
                                              double *d_fa, int64_t *d_w, int8_t *d_st, uint32_t *d_ev, double *d_images,
                                              int32_t *d_n_hits, hipStream_t s, const DiskParams &dp, const DiskRecordsBuf &recs);

// A band of a supersampled frame (lt_api_aa.inc): the frame render_dev_impl is given is the band of the FINE frame, and
// the resolve epilogue of lt_aa.hpp takes the place of the mode's own, writing d_rgb / d_rgba / d_cover as the band's
// OUTPUT rows.
struct AaBand {
    int samples, mode; // S; LT_AA_*
    int W;             // output width
    int64_t rows;      // output rows of the band
    uint8_t *d_cover;  // (rows, W, 4) or NULL
    // A call of several bands: the partition's row blocks (ascending), of which the band is `count` from `first` on.  The
    // whole list is uploaded once per call and every band points into it.  NULL: the band is the partition of `opts`.
    const std::vector<int32_t> *blocks;
    size_t first, count;
};
static int launch_epilogue_aa(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w, const FrameOut &fo,
                              uint64_t *d_stats, hipStream_t s, const DiskParams *disk, const DiskRecordsBuf &recs, const AaBand &aa);

// The three stages of a frame, each launched once in terms of the precision's type.
static int launch_prologue_camera(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w, int64_t n_q,
                                  hipStream_t s)
{
    with_precision(o.precision, [&](auto t) {
        using T = decltype(t);
        k_prologue_camera<T><<<(unsigned)((n_q + 255) / 256), 256, 0, s>>>(c, mc, w.ic<T>(), n_q);
    });
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

// The integrate launch of a frame or a batch: with `disk` the disk's kernels, else the plain ones.
static int launch_integrate_any(const MetricConsts &mc, const lt_opts &o, double lambda_max, const Workspace &w, int64_t n_q,
                                hipStream_t s, uint64_t *kstats, const DiskParams *disk, const DiskRecordsBuf &recs)
{
    if (disk)
        return with_precision(o.precision, [&](auto t) {
            return launch_integrate_disk<decltype(t)>(mc, o, lambda_max, w, n_q, s, kstats, *disk, recs);
        });
    return with_precision(o.precision, [&](auto t) { return launch_integrate<decltype(t)>(mc, o, lambda_max, w, n_q, s, kstats); });
}

// The launch shape the three per-pixel frame epilogues share: launch(T{}, std::bool_constant<HAS_BG>{}, grid), one
// workgroup of EPILOGUE_BLOCK pixels of one row.
template <typename Launch> static void launch_epilogue_rows(const CamConsts &c, const lt_opts &o, const FrameOut &fo, Launch launch)
{
    const bool has_bg = fo.bg != nullptr && (fo.rgb || fo.rgba);
    const dim3 ge((unsigned)((c.W + EPILOGUE_BLOCK - 1) / EPILOGUE_BLOCK), (unsigned)c.rows_local);
    with_precision(o.precision, [&](auto t) {
        if (has_bg) launch(t, std::true_type{}, ge);
        else launch(t, std::false_type{}, ge);
    });
}

// The same for the local rows [row0, row1), in slices of at most 65535 rows (grid.y carries the row within a slice):
// launch(T{}, std::bool_constant<HAS_BG>{}, grid, first row of the slice).
template <typename Launch>
static void launch_epilogue_rows(const CamConsts &c, const lt_opts &o, const FrameOut &fo, int row0, int row1, Launch launch)
{
    const bool has_bg = fo.bg != nullptr && (fo.rgb || fo.rgba);
    with_precision(o.precision, [&](auto t) {
        for (int r = row0; r < row1; r += std::min(row1 - r, 65535)) {
            const dim3 ge((unsigned)((c.W + EPILOGUE_BLOCK - 1) / EPILOGUE_BLOCK), (unsigned)std::min(row1 - r, 65535));
            if (has_bg) launch(t, std::true_type{}, ge, r);
            else launch(t, std::false_type{}, ge, r);
        }
    });
}

// Whether a frame's epilogue is the one that stages background tiles in LDS (opts->bg_sampling, a background is lensed)
static bool epilogue_is_lds(const lt_opts &o, const FrameOut &fo) { return o.bg_sampling == LT_BG_LDS_TILES && fo.bg && (fo.rgb || fo.rgba); }

// k_epilogue_frame over the local rows [row0, row1); the counters stay in the workspace's partial sets
static int launch_epilogue_frame_rows(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w,
                                      const FrameOut &fo, hipStream_t s, int row0, int row1)
{
    launch_epilogue_rows(c, o, fo, row0, row1, [&](auto t, auto bg, dim3 ge, int r0) {
        using T = decltype(t);
        k_epilogue_frame<T, decltype(bg)::value><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, w.fin0<T>(), w.fin1<T>(), fo, r0);
    });
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

static int launch_epilogue_frame(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w,
                                 const FrameOut &fo, uint64_t *d_stats, hipStream_t s, int row0 = 0)
{
    // background tiles staged in LDS when a background is lensed (opts->bg_sampling)
    if (epilogue_is_lds(o, fo)) {
        const unsigned gp = (unsigned)((int64_t)((c.W + 15) / 16) * ((c.rows_local + 15) / 16)); // one 16x16 tile per workgroup
        with_precision(o.precision, [&](auto t) {
            using T = decltype(t);
            k_epilogue_frame_lds<T><<<gp, 256, 0, s>>>(c, mc, w.fin0<T>(), w.fin1<T>(), fo);
        });
    } else if (int rc = launch_epilogue_frame_rows(c, mc, o, w, fo, s, row0, c.rows_local)) // (row0 > 0: the rows before were shaded already, the tail split)
        return rc;
    if (d_stats) k_stats_reduce<<<1, STAT_SLOTS, 0, s>>>(w.partials, (unsigned long long *)d_stats, LT_STAT_BG_TILES_LDS, LT_STAT_BG_TILES_GLOBAL);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

// Pinhole, psi frame and the axis-refine columns' threshold of a camera (image_lens.py:138-139, :210-214), into a
// zero-filled CamConsts.  Returns whether the hole lies in front of the camera.
static bool camera_pinhole(const lt_camera *cam, double axis_refine_frac, CamConsts *c)
{
    memset(c, 0, sizeof(*c));
    c->W = cam->width; c->H = cam->height;
    c->half_W = c->W / 2.0; c->half_H = c->H / 2.0;
    c->fx = (c->W / 2.0) / tan(cam->hfov / 2);
    c->fy = (c->H / 2.0) / tan(cam->vfov / 2);
    bool front;
    psi_frame(cam->psi_y, cam->psi_x, c->d, c->ex, c->ey, &front);
    if (front) {
        c->bh_x_cam = c->d[0] / c->d[2];
        double x_lo = fabs((0 - c->half_W) / c->fx - c->bh_x_cam), x_hi = fabs((c->W - 1 - c->half_W) / c->fx - c->bh_x_cam);
        double m = x_lo > x_hi ? x_lo : x_hi;
        c->refine_thresh = axis_refine_frac * (m > 1e-12 ? m : 1e-12);
    }
    return front;
}

// The camera block of one partition's frame: host arithmetic only.  `owned` / `rows_owned`: the partition's row blocks
// (partition_blocks), `listed`: they are given as a list (a block_owner table, a band); `disk`: a disk frame, which
// traces every row.  The caller adds block_list.  A partition without
// rows (rows_local <= 0) is no error: its block is left without tiles.
static int make_camera(const lt_camera *cam, int kind, const lt_opts &o, const MetricConsts &mc, const std::vector<int32_t> &owned,
                       int64_t rows_owned, bool listed, bool disk, CamConsts *out)
{
    CamConsts &c = *out;
    const bool front = camera_pinhole(cam, o.axis_refine_frac, &c);
    c.row_block = o.row_block; c.n_parts = o.n_parts; c.part = o.part;
    c.rows_local = (int)rows_owned;
    c.loop_around = o.loop_around;
    c.refine_on = front && kind == LT_METRIC_KERR;
    // top/bottom symmetry exactly when the reference applies it (image_lens.py:218-220)
    c.use_tb = !disk && o.tb_symmetry && kind == LT_METRIC_KERR &&
               fabs(cam->theta_obs - M_PI / 2) <= 1e-8 + 1e-5 * (M_PI / 2) && fabs(cam->psi_y) <= 1e-8;
    if (c.use_tb && (o.n_parts != 1 || listed)) return fail(LT_ERR_UNSUPPORTED, "tb_symmetry needs n_parts == 1 and no block_owner table");
    c.trace_rows = c.use_tb ? (c.H + 1) / 2 : c.rows_local;
    c.tiles_x = (c.W + 7) / 8;
    if (c.rows_local <= 0) return LT_OK;
    // (the disks' epilogues carry the whole partition's rows in their launch grid's y dimension; the frame path's epilogue is
    // launched in slices of that many rows, launch_epilogue_rows; a supersampled frame's bands are cut to fit.  Checked
    // before anything is launched)
    if (disk && c.rows_local > 65535)
        return fail(LT_ERR_UNSUPPORTED, "a partition of %d rows exceeds the epilogue's launch grid (65535 rows): split it (n_parts)", c.rows_local);
    const int tiles_y = (c.trace_rows + 7) / 8;
    c.tiles_y = tiles_y;
    // "hot" tile rectangle, queued first: bounds the critical curve (largest impact parameter of a spherical photon
    // orbit: the retrograde equatorial one for Kerr, 3 sqrt(3) M for a = 0), + margin
    if (!front || kind != LT_METRIC_KERR) return LT_OK;
    double a = mc.a, M_ = mc.M;
    double b_max = 3.0 * sqrt(3.0) * M_;
    if (a != 0.0) { // Bardeen: r_ret = 2M (1 + cos(2/3 acos(|a|/M))), xi(r) as in metrics.py:886-887
        double aa = fabs(a);
        double r_ph = 2.0 * M_ * (1.0 + cos(2.0 / 3.0 * acos(aa / M_)));
        double Dl = r_ph * r_ph - 2.0 * M_ * r_ph + aa * aa;
        double xi = (r_ph * r_ph + aa * aa) / aa - 2.0 * r_ph * Dl / (aa * (r_ph - M_));
        if (fabs(xi) > b_max) b_max = fabs(xi);
    }
    b_max = 1.05 * b_max + 0.3 * M_;
    double f0 = 1.0 - 2.0 * M_ / cam->r_obs;
    double sin_al = f0 > 0 ? b_max * sqrt(f0) / cam->r_obs : 1.0;
    if (!(sin_al < 0.98)) return LT_OK;
    double tan_al = sin_al / sqrt(1.0 - sin_al * sin_al);
    double bx = c.d[0] / c.d[2] * c.fx + c.half_W, by = c.d[1] / c.d[2] * c.fy + c.half_H; // BH pixel
    double rx = tan_al * c.fx + 8.0, ry = tan_al * c.fy + 8.0;                             // pixels
    auto clampi = [](double v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); };
    c.hot_x0 = clampi(floor((bx - rx) / 8.0), 0, c.tiles_x);
    c.hot_x1 = clampi(ceil((bx + rx) / 8.0), 0, c.tiles_x);
    // rows: global pixel rows -> this partition's local rows (block-cyclic: about 1/n_parts of them)
    double ly0 = (by - ry) / o.n_parts - o.row_block, ly1 = (by + ry) / o.n_parts + o.row_block;
    if (listed) { // any assignment: local rows of the first / last owned block that touches the band
        ly0 = 1e18; ly1 = -1.0;
        for (size_t i = 0; i < owned.size(); ++i) {
            double g0 = (double)owned[i] * o.row_block, g1 = g0 + o.row_block;
            if (g1 < by - ry || g0 > by + ry) continue;
            if ((double)i * o.row_block < ly0) ly0 = (double)i * o.row_block;
            ly1 = (double)(i + 1) * o.row_block;
        }
        if (ly1 < 0) ly0 = ly1 = 0.0;
    }
    c.hot_y0 = clampi(floor(ly0 / 8.0), 0, tiles_y);
    c.hot_y1 = clampi(ceil(ly1 / 8.0), 0, tiles_y);
    if (c.hot_x1 <= c.hot_x0 || c.hot_y1 <= c.hot_y0) c.hot_x0 = c.hot_x1 = c.hot_y0 = c.hot_y1 = 0;
    // spin-axis strip: +-16 px around the column the BH projects to; then move the rectangle's column range onto the grid with the strip removed
    c.strip_x0 = clampi(floor((bx - 16.0) / 8.0), 0, c.tiles_x);
    c.strip_x1 = clampi(ceil((bx + 16.0) / 8.0), 0, c.tiles_x);
    if (c.strip_x1 < c.strip_x0) c.strip_x1 = c.strip_x0;
    int sw = c.strip_x1 - c.strip_x0;
    auto compact = [&](int x) { return x <= c.strip_x0 ? x : (x - sw > c.strip_x0 ? x - sw : c.strip_x0); };
    c.hot_x0 = compact(c.hot_x0);
    c.hot_x1 = compact(c.hot_x1);
    if (c.hot_x1 <= c.hot_x0) c.hot_x0 = c.hot_x1 = c.hot_y0 = c.hot_y1 = 0;
    return LT_OK;
}

// Block-owner table mode: the partition's block list on the device (uploaded once: again only when it changes).
static int upload_block_list(hipStream_t s, const std::vector<int32_t> &owned, const int32_t **d_list)
{
    StreamSlot *sl;
    int rc = get_slot(s, &sl);
    if (rc) return rc;
    if (sl->blocks_host != owned || !sl->blocks.p) {
        if ((rc = grow(sl->blocks, owned.size() * sizeof(int32_t), s))) return rc;
        HIP_TRY(hipStreamSynchronize(s)); // frames in flight on this stream still read the old list
        HIP_TRY(hipMemcpy(sl->blocks.p, owned.data(), owned.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        sl->blocks_host = owned;
    }
    *d_list = (const int32_t *)sl->blocks.p;
    return LT_OK;
}

// What k_prologue_camera would read for this frame (IcKey).
static IcKey make_ic_key(const CamConsts &c, const std::vector<int32_t> &owned, const MetricConsts &mc, size_t elem, int64_t n_q)
{
    IcKey key;
    key.valid = true;
    memcpy(&key.cam, &c, sizeof(c)); // c was zero-filled before its members were set
    key.cam.block_list = nullptr;
    key.has_blocks = c.block_list != nullptr;
    if (key.has_blocks) key.blocks = owned;
    key.kind = mc.kind; key.obs_ok = mc.obs_ok;
    const double mkey[15] = {mc.M, mc.a, mc.r_obs, mc.theta_obs, mc.R_S, mc.obs_sin_th, mc.obs_cos2, mc.obs_sin2, mc.obs_sqrt_Sigma,
                             mc.obs_sqrt_Delta, mc.obs_g_tt, mc.obs_g_tphi, mc.obs_g_rr, mc.obs_g_thth, mc.obs_g_phiphi};
    memcpy(key.metric, mkey, sizeof(mkey));
    key.elem = elem; key.n_q = n_q;
    return key;
}

// Leaves the slot without a record key unless the frame was enqueued whole (ok).
struct KeyGuard {
    StreamSlot *sl;
    bool ok = false;
    ~KeyGuard() { if (ok) return; std::lock_guard<std::mutex> lk(g_mu); sl->ic_key.valid = false; }
};

// The tail split's join: once the fork event is recorded, the slot's stream waits for whatever the side stream was given
// before the call returns, on every path (grow() and lt_release_stream rely on it).  record() after the side stream's
// last launch, wait() where the user's stream needs its results; a return before either does both here.
struct SideJoin {
    StreamSlot *sl;
    hipStream_t s;
    bool recorded = false, waited = false;
    int record() { HIP_TRY(hipEventRecord(sl->join, sl->side)); recorded = true; return LT_OK; }
    int wait() { HIP_TRY(hipStreamWaitEvent(s, sl->join, 0)); waited = true; return LT_OK; }
    ~SideJoin()
    {
        if (waited) return; // (an error return: g_err keeps the message of what failed)
        if ((!recorded && hipEventRecord(sl->join, sl->side) != hipSuccess) || hipStreamWaitEvent(s, sl->join, 0) != hipSuccess)
            (void)hipStreamSynchronize(sl->side);
    }
};

// disk == NULL: the frame path.  Else the disk frame (lt_render_disk_dev): every row traced, the disk kernels.
// aa != NULL: a band of a supersampled frame, resolved by k_epilogue_aa instead of the mode's epilogue.
static int render_dev_impl(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const float *d_bg,
                           int32_t bg_channels, float *d_fa, uint16_t *d_w, int8_t *d_status, uint32_t *d_steps,
                           float *d_rgb, uint8_t *d_rgba, uint64_t *d_stats, const EventQuad *own_events,
                           const DiskParams *disk = nullptr, const AaBand *aa = nullptr)
{
    int rc = require_device();
    if (rc) return rc;
    if (!cam || !metric || !opts) return fail(LT_ERR_INVALID_ARG, "null camera / metric / opts");
    if (cam->width <= 0 || cam->height <= 0) return fail(LT_ERR_INVALID_ARG, "empty frame %dx%d", cam->width, cam->height);
    if (d_bg && bg_channels != 1 && bg_channels != 3) return fail(LT_ERR_INVALID_ARG, "bg_channels must be 1 or 3");
    lt_opts o = *opts;
    if ((rc = check_opts(metric, &o))) return rc;
    MetricConsts mc;
    if ((rc = make_metric(metric, cam->r_obs, cam->theta_obs, o.h_max, &mc))) return rc;
    count_evals(o.integrator, &mc);

    hipStream_t s = (hipStream_t)o.stream;
    std::vector<int32_t> owned;
    int64_t rows_owned = 0;
    const int32_t *block_list = nullptr;
    if (aa && aa->blocks) { // (the list is the same for every band of the call: uploaded by the first, found unchanged by the others)
        if ((rc = upload_block_list(s, *aa->blocks, &block_list))) return rc;
        block_list += aa->first;
        owned.assign(aa->blocks->begin() + (long)aa->first, aa->blocks->begin() + (long)(aa->first + aa->count));
        rows_owned = aa->rows * aa->samples;
    } else {
        if ((rc = partition_blocks(cam->height, o, &owned, &rows_owned))) return rc;
        if (o.block_owner && !owned.empty() && (rc = upload_block_list(s, owned, &block_list))) return rc;
    }
    CamConsts c;
    if ((rc = make_camera(cam, metric->kind, o, mc, owned, rows_owned, block_list != nullptr, disk != nullptr, &c))) return rc;
    c.block_list = block_list;
    if (c.rows_local <= 0) return LT_OK; // a partition may own no rows
    int64_t n_q = (int64_t)c.tiles_x * c.tiles_y * 64;
    if (n_q / 64 >= (int64_t)1 << 31) // (the prologue decodes a tile's queue position in 32 bits; 2^31 tiles of records would be 6 TB)
        return fail(LT_ERR_INVALID_ARG, "frame of %d x %d tiles: more than 2^31 - 1", c.tiles_x, c.tiles_y);
    double lambda_max = fmax(5000.0, 6.0 * cam->r_obs); // metrics.py:1132

    const size_t elem = elem_size(o.precision);
    Workspace w;
    StreamSlot *slot;
    IcKey held;
    if ((rc = get_workspace(s, (size_t)n_q, elem, &w, &slot, &held))) return rc; // (the slot's key is now cleared)
    IcKey key = make_ic_key(c, owned, mc, elem, n_q);
    const bool reuse = ic_reuse_enabled() && key.same(held);
    KeyGuard guard{slot}; // from here on an error return leaves the slot without a key
    DiskRecordsBuf recs;
    if ((rc = get_disk_records(s, n_q, elem, disk, &recs))) return rc;
    Timer tm;
    if ((rc = tm.begin(o.timing != 0, own_events))) return rc;
    // the epilogue adds its counters into STAT_SLOTS partial sets (workgroup index mod STAT_SLOTS) of the workspace; one
    // small launch behind it folds them into the caller's counters
    FrameOut fo{d_bg, bg_channels, d_fa, d_w, d_status, d_steps, d_rgb, d_rgba, d_stats ? (uint64_t *)w.partials : nullptr};

    // The tail split, decided once per call: the plain Kerr frame of the direct schedule whose epilogue is
    // k_epilogue_frame over every row (no disk, no supersampling band, no top/bottom mirror, no LDS-tiled background), on a
    // stream that is not being captured -- a capture would draw the side stream into the caller's graph --, and without the
    // diagnostic wave stamps, which are dumped per launch.  tail_split_plan decides whether the frame has the rows for it.
    int ty_split = c.tiles_y;
    int64_t pos_split = n_q / 64;
    bool split = false;
    const int split_request = tail_split_request();
    if (split_request != 0 && !disk && !aa && mc.kind == LT_METRIC_KERR && o.schedule == LT_SCHED_DIRECT && !c.use_tb &&
        !epilogue_is_lds(o, fo) && !getenv("LT_STAMPS_FILE")) {
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &capturing) != hipSuccess) {
            (void)hipGetLastError(); // (the legacy stream while another stream captures: no split, and the launches below report what there is to report)
            capturing = hipStreamCaptureStatusActive;
        }
        if (capturing == hipStreamCaptureStatusNone) {
            const int slots = with_precision(o.precision, [&](auto t) { return direct_slots<decltype(t)>(o); });
            split = tail_split_plan(c.tiles_x, c.tiles_y, c.strip_x1 - c.strip_x0, c.hot_y1, slots, split_request, &ty_split, &pos_split);
        }
    }

    if ((rc = tm.mark(0, s))) return rc;
    // (marks 0 and 1 are recorded either way: a reused prologue reports a time near zero, not a stale one)
    if (!reuse && (rc = launch_prologue_camera(c, mc, o, w, n_q, s))) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        slot->ic_key = std::move(key);
        ++(reuse ? g_ic_hits : g_ic_misses);
        ++(split ? g_split_frames : g_whole_frames);
    }
    if ((rc = tm.mark(1, s))) return rc;
    if (split) {
        // user's stream:  record fork . K2a (part A) ......... K3a (rows of part A) . wait join . K3b (the other rows) . reduce
        // side stream:    wait fork . zero head_b . K2b (part B) . record join
        // K2a's grid fills the chip; K2b's workgroups get the wave slots K2a's wavefronts leave as the queue runs dry, K3a
        // starts when K2a has ended and runs beside what is left of K2b.  No wave waits for another and every output is
        // written on the user's stream, K3b's after the join: what the caller may assume on return is what it was.
        // Timing marks: 2 is recorded after the join, so integrate_ms spans K2a and K2b AND the K3a that overlaps them, and
        // epilogue_ms is K3b and the reduce alone.  The three times still tile the frame (their sum is the span from mark 0
        // to mark 3), so a rate derived from integrate_ms can only read lower than the kernel's own, never higher.
        const int64_t n_tiles = n_q / 64;
        const QueuePart part_a{0, pos_split, w.head}, part_b{pos_split, n_tiles - pos_split, w.head_b};
        const int rows_a = std::min(ty_split * 8, c.rows_local);
        if ((rc = slot_side(slot))) return rc;
        HIP_TRY(hipEventRecord(slot->fork, s));
        SideJoin sj{slot, s}; // from here on every return joins the side stream back into `s`
        auto integrate = [&](const QueuePart &part, hipStream_t on) {
            return with_precision(o.precision, [&](auto t) { return launch_integrate<decltype(t)>(mc, o, lambda_max, w, n_q, on, d_stats, &part); });
        };
        if ((rc = integrate(part_a, s))) return rc;
        HIP_TRY(hipStreamWaitEvent(slot->side, slot->fork, 0));
        if ((rc = integrate(part_b, slot->side))) return rc;
        if ((rc = sj.record())) return rc;
        if (rows_a > 0 && (rc = launch_epilogue_frame_rows(c, mc, o, w, fo, s, 0, rows_a))) return rc;
        if ((rc = sj.wait())) return rc;
        if ((rc = tm.mark(2, s))) return rc;
        if ((rc = launch_epilogue_frame(c, mc, o, w, fo, d_stats, s, rows_a))) return rc;
        if ((rc = tm.mark(3, s))) return rc;
        tm.finish();
        guard.ok = true;
        return LT_OK;
    }
    if ((rc = launch_integrate_any(mc, o, lambda_max, w, n_q, s, d_stats, disk, recs))) return rc;
    if ((rc = tm.mark(2, s))) return rc;
    if (aa) rc = launch_epilogue_aa(c, mc, o, w, fo, d_stats, s, disk, recs, *aa);
    else if (!disk) rc = launch_epilogue_frame(c, mc, o, w, fo, d_stats, s);
    else if (disk->max_images) rc = launch_epilogue_disk_images(c, mc, o, w, fo, d_stats, s, *disk, recs);
    else rc = launch_epilogue_disk(c, mc, o, w, fo, d_stats, s, *disk);
    if (rc) return rc;
    if ((rc = tm.mark(3, s))) return rc;
    tm.finish();
    guard.ok = true;
    return LT_OK;
}

extern "C" int lt_render_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const float *d_bg,
                             int32_t bg_channels, float *d_fa, uint16_t *d_w, int8_t *d_status, uint32_t *d_steps,
                             float *d_rgb, uint8_t *d_rgba, uint64_t *d_stats)
{
    return render_dev_impl(cam, metric, opts, d_bg, bg_channels, d_fa, d_w, d_status, d_steps, d_rgb, d_rgba, d_stats,
                           nullptr);
}

// RAII device buffer for the host-pointer entry points
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) { HIP_TRY(hipMalloc(&p, n ? n : 1)); return LT_OK; }
};

// ---- pinned host memory for callers of the host-pointer entry points ---------------------------
// A destination inside such a block is written by DMA straight from the device (PCIe rate); any other
// destination is pageable memory, which the HIP runtime has to pin page by page during the copy.
extern "C" void *lt_host_alloc(size_t bytes)
{
    if (lt_device_count() <= 0) { (void)fail(LT_ERR_NO_DEVICE, "lt_host_alloc: no HIP device visible"); return nullptr; }
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
    if (e != hipSuccess) { (void)fail(LT_ERR_HIP, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); return nullptr; }
    return p;
}

extern "C" int lt_host_free(void *p)
{
    if (!p) return LT_OK;
    HIP_TRY(hipHostFree(p));
    return LT_OK;
}

// The device-side copies of a host-pointer call's arrays: pieces of the slot's ONE grow-only `dev` buffer, so nothing is
// allocated per call once it has reached the frame size.  A call declares each array once -- host pointer, element
// count and size, direction; a null host pointer declares nothing: its device pointer is null and its copies are skipped --, commits
// (one grow, then the inputs' copies in the order declared), asks for device pointers and fetches the outputs.
//
// Device -> host is one asynchronous copy per output, straight into the caller's memory.  Into pinned memory
// (lt_host_alloc) that is a DMA at PCIe rate (measured 55 GB/s: 1.2 ms for a 4096^2 RGBA8 frame).  Into pageable memory
// the HIP runtime pins the destination pages on the fly: 14 ms for the same 64 MiB the first time a buffer is used,
// 1.2 ms when the same buffer is passed again (tools/scratch/hostmem_probe.cpp).  A staging scheme of our own (pinned
// bounce buffer + host copy threads) was built and measured slower than that.
struct Staging {
    static constexpr int MAX_PIECES = 12;
    struct Piece { void *host; size_t count, unit, off; bool input; }; // `count` elements of `unit` bytes
    StreamSlot *sl = nullptr; hipStream_t s = nullptr; // (set by commit)
    Carver cv;
    Piece pieces[MAX_PIECES];
    int n_pieces = 0;
    bool overflow = false; // more than MAX_PIECES declared: commit() refuses
    int add(const void *host, size_t count, size_t unit, bool input)
    {
        if (n_pieces == MAX_PIECES) { overflow = true; return 0; }
        pieces[n_pieces] = {(void *)host, count, unit, host ? cv.take(count * unit) : 0, input};
        return n_pieces++;
    }
    int in(const void *host, size_t count, size_t unit) { return add(host, count, unit, true); }
    int out(void *host, size_t count, size_t unit) { return add(host, count, unit, false); }
    int commit(hipStream_t stream)
    {
        if (overflow) return fail(LT_ERR_INVALID_ARG, "Staging: more than %d arrays declared", MAX_PIECES);
        s = stream;
        int rc = get_slot(s, &sl);
        if (rc || (rc = grow(sl->dev, cv.off, s))) return rc;
        for (int i = 0; i < n_pieces; ++i)
            if (pieces[i].input && pieces[i].host)
                HIP_TRY(hipMemcpyAsync(dev<char>(i), pieces[i].host, pieces[i].count * pieces[i].unit, hipMemcpyHostToDevice, s));
        return LT_OK;
    }
    template <typename P> P *dev(int i) const { return pieces[i].host ? (P *)((char *)sl->dev.p + pieces[i].off) : nullptr; }
    // `count` elements of piece i, from its element `dev_first` on, to element `host_first` of the host array
    int fetch(int i, size_t host_first, size_t dev_first, size_t count) const
    {
        const Piece &pc = pieces[i];
        if (pc.host && count)
            HIP_TRY(hipMemcpyAsync((char *)pc.host + host_first * pc.unit, dev<char>(i) + dev_first * pc.unit, count * pc.unit,
                                   hipMemcpyDeviceToHost, s));
        return LT_OK;
    }
    int fetch(int i) const { return fetch(i, 0, 0, pieces[i].count); }
};

// The arrays of one lt_render call (or of one partition of lt_render_multi) in the slot's buffer: `n` pixels of the
// partition, the background of the whole frame, the counters into st->counters.
struct FrameStaging : Staging {
    int stats, bg, fa, w, status, steps, rgb, rgba;
    void declare(lt_stats *st, const float *h_bg, int32_t bg_channels, size_t n_full, size_t n, float *out_fa, uint16_t *out_w,
                 int8_t *out_status, uint32_t *out_steps, float *out_rgb, uint8_t *out_rgba)
    {
        stats = out(st->counters, LT_STAT_WORDS, 8);
        bg = in(h_bg, n_full, bg_channels * sizeof(float));
        fa = out(out_fa, n, 4); w = out(out_w, n, 2); status = out(out_status, n, 1);
        steps = out(out_steps, n, 4); rgb = out(out_rgb, n, (h_bg ? bg_channels : 3) * 4);
        rgba = out(out_rgba, n, 4);
    }
    // Once committed: zeroes the counters and renders with the slot's private timing events (concurrent
    // lt_render_dev(timing = 1) callers keep theirs).  dp: a disk with its device-side outputs, or NULL.
    int render(const lt_camera *cam, const lt_metric *metric, lt_opts o, int32_t bg_channels, const DiskParams *dp)
    {
        int rc;
        HIP_TRY(hipMemsetAsync(dev<char>(stats), 0, LT_STAT_WORDS * 8, s));
        if ((rc = slot_events(sl))) return rc;
        o.timing = 0;
        return render_dev_impl(cam, metric, &o, dev<const float>(bg), bg_channels, dev<float>(fa), dev<uint16_t>(w), dev<int8_t>(status),
                               dev<uint32_t>(steps), dev<float>(rgb), dev<uint8_t>(rgba), dev<uint64_t>(stats), &sl->own, dp);
    }
    // small and first to be consumed go first; the framebuffer follows
    std::array<int, 6> fetch_order() const { return {rgba, fa, w, status, steps, rgb}; }
    // the three stage times of the frame this slot rendered last (after its stream was synchronised)
    int times(float ms[3]) const
    {
        for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], sl->own.e[i], sl->own.e[i + 1]));
        return LT_OK;
    }
};

// lt_render, and with `disk` lt_render_disk (out_disk: (R, W, 3) float32 host array or NULL) or, with
// disk->max_images > 0, lt_render_disk_images (out_images (R, W, max_images, 3) float32, out_n_hits (R, W), or NULL)
static int render_host_impl(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const float *bg,
                            int32_t bg_channels, float *out_fa, uint16_t *out_w, int8_t *out_status, uint32_t *out_steps,
                            float *out_rgb, uint8_t *out_rgba, lt_stats *stats, const DiskParams *disk = nullptr,
                            float *out_disk = nullptr, float *out_images = nullptr, uint8_t *out_n_hits = nullptr,
                            float *out_pol = nullptr)
{
    int rc = require_device();
    if (rc) return rc;
    if (!cam || !metric || !opts) return fail(LT_ERR_INVALID_ARG, "null camera / metric / opts");
    lt_opts o = *opts;
    if ((rc = check_opts(metric, &o))) return rc;
    if (cam->height <= 0 || cam->width <= 0) return fail(LT_ERR_INVALID_ARG, "bad frame / partition");
    int64_t rows = 0;
    if ((rc = partition_blocks(cam->height, o, nullptr, &rows))) return rc;
    if (bg && bg_channels != 1 && bg_channels != 3) return fail(LT_ERR_INVALID_ARG, "bg_channels must be 1 or 3");
    const size_t n = (size_t)rows * cam->width;
    lt_stats st;
    memset(&st, 0, sizeof(st));
    FrameStaging fs;
    fs.declare(&st, bg, bg_channels, (size_t)cam->height * cam->width, n, out_fa, out_w, out_status, out_steps, out_rgb, out_rgba);
    const int i_disk = fs.out(out_disk, n, 3 * 4);
    const int i_img = fs.out(out_images, n, disk ? (size_t)disk->max_images * disk->image_words() * 4 : 0), i_hits = fs.out(out_n_hits, n, 1);
    const int i_pol = fs.out(out_pol, n, disk ? (size_t)disk->max_images * 16 : 0);
    if ((rc = fs.commit((hipStream_t)o.stream))) return rc;
    DiskParams dp{};
    if (disk) {
        dp = *disk;
        dp.d_disk = fs.dev<float>(i_disk); dp.d_images = fs.dev<float>(i_img); dp.d_n_hits = fs.dev<uint8_t>(i_hits);
        dp.d_pol = fs.dev<float>(i_pol);
    }
    if ((rc = fs.render(cam, metric, o, bg_channels, disk ? &dp : nullptr))) return rc;
    for (int i : fs.fetch_order()) if ((rc = fs.fetch(i))) return rc;
    if ((rc = fs.fetch(i_disk)) || (rc = fs.fetch(i_img)) || (rc = fs.fetch(i_hits)) || (rc = fs.fetch(i_pol)) ||
        (rc = fs.fetch(fs.stats)))
        return rc;
    HIP_TRY(hipStreamSynchronize(fs.s));
    if (rows > 0) {
        float ms[3] = {0, 0, 0};
        if ((rc = fs.times(ms))) return rc;
        st.prologue_ms = ms[0]; st.integrate_ms = ms[1]; st.epilogue_ms = ms[2];
    }
    if (stats) *stats = st;
    return LT_OK;
}

extern "C" int lt_render(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const float *bg,
                         int32_t bg_channels, float *out_fa, uint16_t *out_w, int8_t *out_status, uint32_t *out_steps,
                         float *out_rgb, uint8_t *out_rgba, lt_stats *stats)
{
    return render_host_impl(cam, metric, opts, bg, bg_channels, out_fa, out_w, out_status, out_steps, out_rgb, out_rgba, stats);
}

// ---- one frame on several devices from one process ----------------------------------------------
static int multi_stream(int dev, int idx, hipStream_t *out)
{
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto &m : g_multi_streams)
        if (m.dev == dev && m.idx == idx) { *out = m.s; return LT_OK; }
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    g_multi_streams.push_back({dev, idx, s});
    *out = s;
    return LT_OK;
}

extern "C" int lt_render_multi(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, int32_t n_gpus,
                               const int32_t *devices, const float *bg, int32_t bg_channels, float *out_fa,
                               uint16_t *out_w, int8_t *out_status, uint32_t *out_steps, float *out_rgb,
                               uint8_t *out_rgba, lt_stats *stats)
{
    int rc = require_device();
    if (rc) return rc;
    if (!cam || !metric || !opts) return fail(LT_ERR_INVALID_ARG, "null camera / metric / opts");
    if (n_gpus < 1 || n_gpus > 64) return fail(LT_ERR_INVALID_ARG, "n_gpus = %d", n_gpus);
    if (cam->width <= 0 || cam->height <= 0) return fail(LT_ERR_INVALID_ARG, "empty frame %dx%d", cam->width, cam->height);
    if (bg && bg_channels != 1 && bg_channels != 3) return fail(LT_ERR_INVALID_ARG, "bg_channels must be 1 or 3");
    lt_opts o = *opts;
    if ((rc = check_opts(metric, &o))) return rc;
    const int n_dev = lt_device_count();
    std::vector<int> dev((size_t)n_gpus);
    for (int p = 0; p < n_gpus; ++p) {
        dev[(size_t)p] = devices ? devices[p] : p;
        if (dev[(size_t)p] < 0 || dev[(size_t)p] >= n_dev)
            return fail(LT_ERR_INVALID_ARG, "partition %d wants device %d but %d device(s) are visible", p, dev[(size_t)p], n_dev);
    }
    int keep = 0;
    HIP_TRY(hipGetDevice(&keep));
    struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{keep};

    const int W = cam->width, H = cam->height;
    struct Part { FrameStaging fs; int64_t rows; };
    std::vector<Part> parts((size_t)n_gpus);
    std::vector<lt_stats> each((size_t)n_gpus); // destination of asynchronous copies: must outlive the drain below
    // Any return before the end leaves kernels and device-to-host copies of other partitions in flight, writing the
    // caller's arrays and `each`: drain every stream that was handed work before the frame (or the error) is returned.
    struct Drain {
        std::vector<std::pair<int, hipStream_t>> used;
        bool done = false;
        ~Drain() { if (!done) for (auto &u : used) { (void)hipSetDevice(u.first); (void)hipStreamSynchronize(u.second); } }
    } drain;
    // 1. launch every partition (asynchronous): all devices compute at the same time
    for (int p = 0; p < n_gpus; ++p) {
        Part &P = parts[(size_t)p];
        hipStream_t ps;
        HIP_TRY(hipSetDevice(dev[(size_t)p]));
        if ((rc = multi_stream(dev[(size_t)p], p, &ps))) return rc;
        drain.used.push_back({dev[(size_t)p], ps});
        P.rows = lt_local_rows(H, o.row_block, n_gpus, p);
        memset(&each[(size_t)p], 0, sizeof(lt_stats));
        P.fs.declare(&each[(size_t)p], bg, bg_channels, (size_t)W * H, (size_t)P.rows * W, out_fa, out_w, out_status, out_steps,
                     out_rgb, out_rgba);
        lt_opts op = o;
        op.n_parts = n_gpus; op.part = p; op.stream = (void *)ps;
        op.block_owner = nullptr; op.n_blocks = 0; // lt_render_multi partitions block-cyclically
        if ((rc = P.fs.commit(ps)) || (rc = P.fs.render(cam, metric, op, bg_channels, nullptr))) return rc;
    }
    // 2. every device copies its row blocks to their place in the caller's full-frame arrays
    lt_stats total;
    memset(&total, 0, sizeof(total));
    for (int p = 0; p < n_gpus; ++p) {
        Part &P = parts[(size_t)p];
        HIP_TRY(hipSetDevice(dev[(size_t)p]));
        for (int i : P.fs.fetch_order()) {
            for (int64_t l0 = 0; l0 < P.rows; l0 += o.row_block) { // (elements are pixels: W of them per row)
                int64_t g0 = lt_global_row(l0, o.row_block, n_gpus, p);
                int64_t nr = P.rows - l0 < o.row_block ? P.rows - l0 : o.row_block;
                if ((rc = P.fs.fetch(i, (size_t)g0 * W, (size_t)l0 * W, (size_t)nr * W))) return rc;
            }
        }
        if ((rc = P.fs.fetch(P.fs.stats))) return rc;
    }
    for (int p = 0; p < n_gpus; ++p) {
        Part &P = parts[(size_t)p];
        HIP_TRY(hipSetDevice(dev[(size_t)p]));
        HIP_TRY(hipStreamSynchronize(P.fs.s));
        for (int i = 0; i < LT_STAT_WORDS; ++i) total.counters[i] += each[(size_t)p].counters[i];
        if (P.rows > 0) {
            float ms[3] = {0, 0, 0};
            if ((rc = P.fs.times(ms))) return rc;
            if (ms[0] > total.prologue_ms) total.prologue_ms = ms[0];
            if (ms[1] > total.integrate_ms) total.integrate_ms = ms[1];
            if (ms[2] > total.epilogue_ms) total.epilogue_ms = ms[2];
        }
    }
    drain.done = true; // every stream was synchronised above
    if (stats) *stats = total;
    return LT_OK;
}

// ---------------------------------------------------------------------------------------------
// array-in / array-out twins
// ---------------------------------------------------------------------------------------------
// disk != NULL: lt_trace_batch_kerr_disk (out_disk (n, 3) float64 or NULL), or with disk->max_images > 0
// lt_trace_batch_kerr_disk_images (out_images (n, max_images, 3) float64, out_n_hits (n) int32, or NULL)
static int trace_batch(const MetricConsts &mc, lt_opts &o, double lambda_max, const double *alphas, const double *thetas,
                       const uint8_t *refines, int64_t n, double *out_fa, int64_t *out_w, int8_t *out_status,
                       uint32_t *out_evals, const DiskParams *disk = nullptr, double *out_disk = nullptr,
                       double *out_images = nullptr, int32_t *out_n_hits = nullptr, double *out_pol = nullptr,
                       bool general_only = false)
{
    int rc;
    if (n < 0) return fail(LT_ERR_INVALID_ARG, "negative ray count");
    if (n == 0) return LT_OK; // image_lens.py:163-166: empty input is legal
    if (!alphas || !out_fa || !out_w) return fail(LT_ERR_INVALID_ARG, "null alphas / out_fa / out_w");
    if (mc.kind == LT_METRIC_KERR && !thetas) return fail(LT_ERR_INVALID_ARG, "Kerr needs thetas");
    int64_t n_q = (n + 63) / 64 * 64;
    const size_t elem = elem_size(o.precision);
    // The twins are synchronous calls on the default stream, like the reference's ("no async").  Records
    // and staging buffers belong to the (device, default stream) slot, so they never alias what an lt_render_dev
    // call on another stream is using, and nothing is allocated per call once they have grown.
    hipStream_t s = nullptr;
    Workspace w;
    if ((rc = get_workspace(s, (size_t)n_q, elem, &w))) return rc;
    DiskRecordsBuf recs;
    if ((rc = get_disk_records(s, n_q, elem, disk, &recs))) return rc;
    Staging st;
    const int i_al = st.in(alphas, n, 8), i_th = st.in(thetas, n, 8), i_ref = st.in(refines, n, 1);
    const int i_fa = st.out(out_fa, n, 8), i_w = st.out(out_w, n, 8), i_st = st.out(out_status, n, 1), i_ev = st.out(out_evals, n, 4);
    const int i_disk = st.out(out_disk, n, 3 * 8);
    const int i_img = st.out(out_images, n, disk ? (size_t)disk->max_images * disk->image_words() * 8 : 0), i_hits = st.out(out_n_hits, n, 4);
    const int i_pol = st.out(out_pol, n, disk ? (size_t)disk->max_images * 32 : 0);
    if ((rc = st.commit(s))) return rc;
    double *d_fa = st.dev<double>(i_fa); int64_t *d_w = st.dev<int64_t>(i_w);
    int8_t *d_st = st.dev<int8_t>(i_st); uint32_t *d_ev = st.dev<uint32_t>(i_ev);
    with_precision(o.precision, [&](auto t) {
        using T = decltype(t);
        k_prologue_arrays<T><<<(unsigned)((n_q + 255) / 256), 256, 0, s>>>(mc, st.dev<const double>(i_al), st.dev<const double>(i_th),
                                                                          st.dev<const uint8_t>(i_ref), n, w.ic<T>(), n_q);
    });
    HIP_TRY(hipGetLastError());
    if (general_only) {
        with_precision(o.precision, [&](auto t) {
            using T = decltype(t);
            k_kerr_general_only<T><<<(unsigned)(n_q / 64), 64, 0, s>>>(make_kerr<T>(mc, lambda_max, o.h_max), w.ic<T>(), w.fin0<T>(), w.fin1<T>(), n_q);
        });
        HIP_TRY(hipGetLastError());
    } else if ((rc = launch_integrate_any(mc, o, lambda_max, w, n_q, s, nullptr, disk, recs))) return rc;
    DiskParams dp_batch{};
    if (disk) { dp_batch = *disk; dp_batch.d_pol = st.dev<double>(i_pol); disk = &dp_batch; }
    if (disk && disk->max_images) {
        if ((rc = launch_epilogue_arrays_disk_images(mc, o, w, n, d_fa, d_w, d_st, d_ev, st.dev<double>(i_img), st.dev<int32_t>(i_hits), s,
                                                     *disk, recs)))
            return rc;
    } else {
        const unsigned gn = (unsigned)((n + 255) / 256);
        if (disk)
            with_precision(o.precision, [&](auto t) {
                using T = decltype(t);
                k_epilogue_arrays_disk<T><<<gn, 256, 0, s>>>(mc, DiskShade{mc.M, mc.a, disk->r_in, disk->q, disk->exposure}, w.fin0<T>(),
                                                             w.fin1<T>(), n, d_fa, d_w, d_st, st.dev<double>(i_disk), d_ev);
            });
        else
            with_precision(o.precision, [&](auto t) {
                using T = decltype(t);
                k_epilogue_arrays<T><<<gn, 256, 0, s>>>(mc, w.fin0<T>(), w.fin1<T>(), n, d_fa, d_w, d_st, d_ev);
            });
    }
    HIP_TRY(hipGetLastError());
    for (int i : {i_fa, i_w, i_st, i_ev, i_disk, i_img, i_hits, i_pol}) if ((rc = st.fetch(i))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return LT_OK;
}

extern "C" int lt_trace_batch_schw(double M, double r_obs, const double *alphas, int64_t n, double phi_max, double h_max,
                                   int precision, double *out_fa, int64_t *out_w, int8_t *out_status, uint32_t *out_rhs_evals)
{
    int rc = require_device();
    if (rc) return rc;
    lt_metric m{LT_METRIC_SCHWARZSCHILD, 0, M, 0.0};
    lt_opts o;
    lt_default_opts(&o);
    o.precision = precision; o.phi_max = phi_max; o.h_max = h_max;
    if ((rc = check_opts(&m, &o))) return rc;
    MetricConsts mc;
    if ((rc = make_metric(&m, r_obs, M_PI / 2, o.h_max, &mc))) return rc;
    return trace_batch(mc, o, 0.0, alphas, nullptr, nullptr, n, out_fa, out_w, out_status, out_rhs_evals);
}

// What the Kerr batch twins share: default options with the caller's three, the checks, the metric block.
static int kerr_batch_setup(const lt_metric *m, double r_obs, double theta_obs, int integrator, int precision, int schedule,
                            lt_opts *o, MetricConsts *mc)
{
    int rc;
    lt_default_opts(o);
    o->integrator = integrator; o->precision = precision; o->schedule = schedule;
    if ((rc = check_opts(m, o)) || (rc = make_metric(m, r_obs, theta_obs, 0.0, mc))) return rc;
    count_evals(integrator, mc);
    return LT_OK;
}

extern "C" int lt_trace_batch_kerr(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                   double theta_obs, double lambda_max, const uint8_t *axis_refines, int integrator,
                                   int precision, int schedule, int64_t n, double *out_fa, int64_t *out_w,
                                   int8_t *out_status, uint32_t *out_rhs_evals)
{
    int rc = require_device();
    if (rc) return rc;
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    lt_opts o;
    MetricConsts mc;
    if ((rc = kerr_batch_setup(&m, r_obs, theta_obs, integrator, precision, schedule, &o, &mc))) return rc;
    return trace_batch(mc, o, lambda_max, alphas, thetas, axis_refines, n, out_fa, out_w, out_status, out_rhs_evals);
}

// lt_trace_batch_kerr (fixed-step RK4) by the general iteration alone: no streak, no ghost lanes.
extern "C" int lt_trace_batch_kerr_general_probe(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                                 double theta_obs, double lambda_max, const uint8_t *axis_refines, int precision,
                                                 int64_t n, double *out_fa, int64_t *out_w, int8_t *out_status,
                                                 uint32_t *out_rhs_evals)
{
    int rc = require_device();
    if (rc) return rc;
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    lt_opts o;
    MetricConsts mc;
    if ((rc = kerr_batch_setup(&m, r_obs, theta_obs, LT_INTEGRATOR_RK4, precision, LT_SCHED_DIRECT, &o, &mc))) return rc;
    return trace_batch(mc, o, lambda_max, alphas, thetas, axis_refines, n, out_fa, out_w, out_status, out_rhs_evals, nullptr, nullptr,
                       nullptr, nullptr, nullptr, true);
}

extern "C" int lt_kerr_rhs_probe(double M, double a, const double *states, const double *p_phi, int64_t n, int precision,
                                 double *out)
{
    int rc = require_device();
    if (rc) return rc;
    if (n <= 0) return LT_OK;
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    MetricConsts mc;
    if ((rc = make_metric(&m, 50.0, M_PI / 2, 0.0, &mc))) return rc;
    DevBuf ds, dp, dout;
    if ((rc = ds.alloc(n * 40)) || (rc = dp.alloc(n * 8)) || (rc = dout.alloc(n * 40))) return rc;
    HIP_TRY(hipMemcpy(ds.p, states, n * 40, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dp.p, p_phi, n * 8, hipMemcpyHostToDevice));
    with_precision(precision, [&](auto t) {
        using T = decltype(t);
        k_kerr_rhs_probe<T><<<(unsigned)((n + 63) / 64), 64>>>(make_kerr<T>(mc, 5000.0, 1.0), (const double *)ds.p, (const double *)dp.p, n,
                                                               (double *)dout.p);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.p, n * 40, hipMemcpyDeviceToHost));
    return LT_OK;
}

// Every float32 with bit pattern bits_lo + i, i < n, through both forms of M<float>::sincos; out as in lt_sincos_q1_probe.
__global__ void k_sincos_q1_probe(uint32_t bits_lo, uint32_t n, unsigned long long *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t bits = bits_lo + i;
    const float x = __uint_as_float(bits);
    float s0, c0, s1, c1;
    M<float>::sincos(x, s0, c0);
    M<float>::sincos_q1(x, s1, c1);
    if ((__float_as_uint(s0) != __float_as_uint(s1)) | (__float_as_uint(c0) != __float_as_uint(c1))) {
        atomicAdd(&out[1], 1ull);
        atomicMin(&out[3], (unsigned long long)bits);
    }
    if (__builtin_rintf(x * 0.636619772367581343f) != 1.0f) atomicAdd(&out[2], 1ull);
}

extern "C" int lt_sincos_q1_probe(uint32_t bits_lo, uint32_t bits_hi, uint64_t out[4], float band[2])
{
    int rc = require_device();
    if (rc) return rc;
    if (!out || bits_hi < bits_lo || bits_hi - bits_lo >= (1u << 30)) return fail(LT_ERR_INVALID_ARG, "bad sincos probe range");
    const uint32_t n = bits_hi - bits_lo + 1;
    DevBuf d;
    if ((rc = d.alloc(4 * sizeof(uint64_t)))) return rc;
    const uint64_t init[4] = {n, 0, 0, ~0ull};
    HIP_TRY(hipMemcpy(d.p, init, sizeof(init), hipMemcpyHostToDevice));
    k_sincos_q1_probe<<<(n + 255) / 256, 256>>>(bits_lo, n, (unsigned long long *)d.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d.p, sizeof(init), hipMemcpyDeviceToHost));
    if (band) { band[0] = M<float>::EQ_BAND_LO; band[1] = M<float>::EQ_BAND_HI; }
    return LT_OK;
}

extern "C" int lt_kerr_rhs_form_probe(double M, double a, const double *states, const double *p_phi, int64_t n, int precision,
                                      int form, double *out)
{
    int rc = require_device();
    if (rc) return rc;
    if (form < 0 || form > 3 || (form >= 2 && precision != 32)) return fail(LT_ERR_INVALID_ARG, "right-hand side form %d (float%d)", form, precision);
    if (n <= 0) return LT_OK;
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    MetricConsts mc;
    if ((rc = make_metric(&m, 50.0, M_PI / 2, 0.0, &mc))) return rc;
    DevBuf ds, dp, dout;
    if ((rc = ds.alloc(n * 40)) || (rc = dp.alloc(n * 8)) || (rc = dout.alloc(n * 40))) return rc;
    HIP_TRY(hipMemcpy(ds.p, states, n * 40, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dp.p, p_phi, n * 8, hipMemcpyHostToDevice));
    with_precision(precision, [&](auto t) {
        using T = decltype(t);
        k_kerr_rhs_form_probe<T><<<(unsigned)((n + 63) / 64), 64>>>(make_kerr<T>(mc, 5000.0, 1.0), (const double *)ds.p, (const double *)dp.p,
                                                                    n, form, (double *)dout.p);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.p, n * 40, hipMemcpyDeviceToHost));
    return LT_OK;
}

extern "C" int lt_kerr_step_probe(double M, double a, const double *states, const double *p_phi, const uint8_t *refine,
                                  const double *h, int64_t n, int precision, int form, double *out_states, double *out_min_r,
                                  double *out_max_d, double *out_cs)
{
    int rc = require_device();
    if (rc) return rc;
    if (form < 0 || form > 3 || (form >= 2 && precision != 32)) return fail(LT_ERR_INVALID_ARG, "step form %d (float%d)", form, precision);
    if (n <= 0) return LT_OK;
    if (!states || !p_phi || !refine || !h || !out_states || !out_min_r || !out_max_d) return fail(LT_ERR_INVALID_ARG, "null pointer");
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    MetricConsts mc;
    if ((rc = make_metric(&m, 50.0, M_PI / 2, 0.0, &mc))) return rc;
    DevBuf ds, dp, dr, dh, dos, dmr, dmd, dcs;
    if ((rc = ds.alloc(n * 40)) || (rc = dp.alloc(n * 8)) || (rc = dr.alloc(n)) || (rc = dh.alloc(n * 8)) || (rc = dos.alloc(n * 40)) ||
        (rc = dmr.alloc(n * 8)) || (rc = dmd.alloc(n * 8)) || (rc = dcs.alloc(n * 16))) return rc;
    HIP_TRY(hipMemcpy(ds.p, states, n * 40, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dp.p, p_phi, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dr.p, refine, n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dh.p, h, n * 8, hipMemcpyHostToDevice));
    with_precision(precision, [&](auto t) {
        using T = decltype(t);
        k_kerr_step_probe<T><<<(unsigned)((n + 63) / 64), 64>>>(make_kerr<T>(mc, 5000.0, 1.0), (const double *)ds.p, (const double *)dp.p,
                                                                (const uint8_t *)dr.p, (const double *)dh.p, n, form, (double *)dos.p,
                                                                (double *)dmr.p, (double *)dmd.p, (double *)dcs.p);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_states, dos.p, n * 40, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_min_r, dmr.p, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_max_d, dmd.p, n * 8, hipMemcpyDeviceToHost));
    if (out_cs) HIP_TRY(hipMemcpy(out_cs, dcs.p, n * 16, hipMemcpyDeviceToHost));
    return LT_OK;
}

// ---- the DP45 integrator block by block ----------------------------------------------------------------------------------
// Device copy of a host array (src may be NULL: nothing allocated), and an output buffer with its way back.
static int probe_upload(DevBuf &d, const void *src, size_t bytes)
{
    if (!src) return LT_OK;
    int rc = d.alloc(bytes);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    return LT_OK;
}
static int probe_download(void *dst, const DevBuf &d, size_t bytes)
{
    if (dst) HIP_TRY(hipMemcpy(dst, d.p, bytes, hipMemcpyDeviceToHost));
    return LT_OK;
}

static int dp45_probe_consts(double M, double a, double r_obs, double lambda_max, KerrConsts<double> *k)
{
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    MetricConsts mc;
    int rc = make_metric(&m, r_obs, M_PI / 2, 0.0, &mc);
    if (rc) return rc;
    *k = make_kerr<double>(mc, lambda_max, 1.0);
    return LT_OK;
}

extern "C" int lt_dp45_attempt_probe(double M, double a, double r_obs, double lambda_max, const double *states,
                                     const double *p_phi, const uint8_t *refine, const double *k1, const double *sc0,
                                     const double *h, int64_t n, int exact, int checked, double *out_next, double *out_k7,
                                     double *out_sc, double *out_err_sq, double *out_min_r, double *out_max_d)
{
    int rc = require_device();
    if (rc) return rc;
    if (n <= 0) return LT_OK;
    if (!states || !p_phi || !refine || !h || !out_next || !out_k7 || !out_sc || !out_err_sq || !out_min_r || !out_max_d)
        return fail(LT_ERR_INVALID_ARG, "null pointer");
    KerrConsts<double> k;
    if ((rc = dp45_probe_consts(M, a, r_obs, lambda_max, &k))) return rc;
    DevBuf ds, dp, dr, dk, dc, dh, on, ok7, osc, oe, omr, omd;
    if ((rc = probe_upload(ds, states, n * 40)) || (rc = probe_upload(dp, p_phi, n * 8)) || (rc = probe_upload(dr, refine, n)) ||
        (rc = probe_upload(dk, k1, n * 40)) || (rc = probe_upload(dc, sc0, n * 16)) || (rc = probe_upload(dh, h, n * 8)) ||
        (rc = on.alloc(n * 40)) || (rc = ok7.alloc(n * 40)) || (rc = osc.alloc(n * 16)) || (rc = oe.alloc(n * 8)) ||
        (rc = omr.alloc(n * 8)) || (rc = omd.alloc(n * 8))) return rc;
    auto launch = [&](auto ex, auto ch) {
        k_dp45_attempt_probe<decltype(ex)::value, decltype(ch)::value><<<(unsigned)((n + 63) / 64), 64>>>(
            k, (const double *)ds.p, (const double *)dp.p, (const uint8_t *)dr.p, (const double *)dk.p, (const double *)dc.p,
            (const double *)dh.p, n, (double *)on.p, (double *)ok7.p, (double *)osc.p, (double *)oe.p, (double *)omr.p, (double *)omd.p);
    };
    if (exact) { if (checked) launch(std::true_type{}, std::true_type{}); else launch(std::true_type{}, std::false_type{}); }
    else { if (checked) launch(std::false_type{}, std::true_type{}); else launch(std::false_type{}, std::false_type{}); }
    HIP_TRY(hipGetLastError());
    if ((rc = probe_download(out_next, on, n * 40)) || (rc = probe_download(out_k7, ok7, n * 40)) || (rc = probe_download(out_sc, osc, n * 16)) ||
        (rc = probe_download(out_err_sq, oe, n * 8)) || (rc = probe_download(out_min_r, omr, n * 8)) || (rc = probe_download(out_max_d, omd, n * 8)))
        return rc;
    return LT_OK;
}

extern "C" int lt_dp45_advance_probe(double M, double a, double r_obs, double lambda_max, const double *states,
                                     const double *p_phi, const uint8_t *refine, const double *k1, const double *sc0,
                                     const double *h, const double *lam, const uint32_t *steps, int64_t n, int exact,
                                     int n_attempts, double *out_states, double *out_k1, double *out_misc, int32_t *out_int)
{
    int rc = require_device();
    if (rc) return rc;
    if (n <= 0) return LT_OK;
    if (n_attempts < 1) return fail(LT_ERR_INVALID_ARG, "n_attempts must be at least 1");
    if (!states || !p_phi || !refine || !h || !out_states || !out_k1 || !out_misc || !out_int) return fail(LT_ERR_INVALID_ARG, "null pointer");
    KerrConsts<double> k;
    if ((rc = dp45_probe_consts(M, a, r_obs, lambda_max, &k))) return rc;
    DevBuf ds, dp, dr, dk, dc, dh, dl, dst, os, ok1, om, oi;
    if ((rc = probe_upload(ds, states, n * 40)) || (rc = probe_upload(dp, p_phi, n * 8)) || (rc = probe_upload(dr, refine, n)) ||
        (rc = probe_upload(dk, k1, n * 40)) || (rc = probe_upload(dc, sc0, n * 16)) || (rc = probe_upload(dh, h, n * 8)) ||
        (rc = probe_upload(dl, lam, n * 8)) || (rc = probe_upload(dst, steps, n * 4)) || (rc = os.alloc(n * 40)) ||
        (rc = ok1.alloc(n * 40)) || (rc = om.alloc(n * 32)) || (rc = oi.alloc(n * 12))) return rc;
    auto launch = [&](auto ex) {
        k_dp45_advance_probe<decltype(ex)::value><<<(unsigned)((n + 63) / 64), 64>>>(
            k, (const double *)ds.p, (const double *)dp.p, (const uint8_t *)dr.p, (const double *)dk.p, (const double *)dc.p,
            (const double *)dh.p, (const double *)dl.p, (const uint32_t *)dst.p, n, n_attempts, (double *)os.p, (double *)ok1.p,
            (double *)om.p, (int32_t *)oi.p);
    };
    if (exact) launch(std::true_type{}); else launch(std::false_type{});
    HIP_TRY(hipGetLastError());
    if ((rc = probe_download(out_states, os, n * 40)) || (rc = probe_download(out_k1, ok1, n * 40)) ||
        (rc = probe_download(out_misc, om, n * 32)) || (rc = probe_download(out_int, oi, n * 12))) return rc;
    return LT_OK;
}

extern "C" int lt_dp45_controller_probe(int exact, const double *err_sq, const double *h, int64_t n, uint8_t *out_reject,
                                        double *out_h)
{
    int rc = require_device();
    if (rc) return rc;
    if (n <= 0) return LT_OK;
    if (!err_sq || !h || !out_reject || !out_h) return fail(LT_ERR_INVALID_ARG, "null pointer");
    DevBuf de, dh, orj, oh;
    if ((rc = probe_upload(de, err_sq, n * 8)) || (rc = probe_upload(dh, h, n * 8)) || (rc = orj.alloc(n)) || (rc = oh.alloc(n * 8))) return rc;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (exact) k_dp45_controller_probe<true><<<grid, 256>>>((const double *)de.p, (const double *)dh.p, n, (uint8_t *)orj.p, (double *)oh.p);
    else k_dp45_controller_probe<false><<<grid, 256>>>((const double *)de.p, (const double *)dh.p, n, (uint8_t *)orj.p, (double *)oh.p);
    HIP_TRY(hipGetLastError());
    if ((rc = probe_download(out_reject, orj, n)) || (rc = probe_download(out_h, oh, n * 8))) return rc;
    return LT_OK;
}

// ---- a ray's two ends and the RK4 loop body ------------------------------------------------------------------------------
// (n,4) records of precision T on the device <-> (n,4) float64 on the host.
template <typename T> static int probe_upload_recs(DevBuf &d, const double *src, int64_t n)
{
    std::vector<T> h((size_t)n * 4);
    for (size_t j = 0; j < h.size(); ++j) h[j] = (T)src[j];
    return probe_upload(d, h.data(), h.size() * sizeof(T));
}
template <typename T> static int probe_download_recs(double *dst, const DevBuf &d, int64_t n)
{
    std::vector<T> h((size_t)n * 4);
    int rc = probe_download(h.data(), d, h.size() * sizeof(T));
    for (size_t j = 0; j < h.size(); ++j) dst[j] = (double)h[j];
    return rc;
}

extern "C" int lt_ic_probe(int kind, double M, double a, double r_obs, double theta_obs, const double *alphas,
                           const double *thetas, const uint8_t *refines, int64_t n, int precision, double *out_records)
{
    int rc = require_device();
    if (rc) return rc;
    if (precision != 32 && precision != 64) return fail(LT_ERR_INVALID_ARG, "precision must be 32 or 64");
    if (n <= 0) return LT_OK;
    if (!alphas || !out_records || (kind == LT_METRIC_KERR && !thetas)) return fail(LT_ERR_INVALID_ARG, "null pointer");
    lt_metric m{kind, 0, M, a};
    MetricConsts mc;
    if ((rc = make_metric(&m, r_obs, theta_obs, 0.0, &mc))) return rc;
    const int64_t n_q = (n + 63) / 64 * 64;
    DevBuf da, dt, dr, dic;
    if ((rc = probe_upload(da, alphas, n * 8)) || (rc = probe_upload(dt, thetas, n * 8)) || (rc = probe_upload(dr, refines, n)) ||
        (rc = dic.alloc((size_t)n_q * 4 * elem_size(precision)))) return rc;
    with_precision(precision, [&](auto t) {
        using T = decltype(t);
        k_prologue_arrays<T><<<(unsigned)((n_q + 255) / 256), 256>>>(mc, (const double *)da.p, (const double *)dt.p, (const uint8_t *)dr.p, n,
                                                                     (typename Vec4<T>::type *)dic.p, n_q);
    });
    HIP_TRY(hipGetLastError());
    return with_precision(precision, [&](auto t) { return probe_download_recs<decltype(t)>(out_records, dic, n_q); });
}

extern "C" int lt_rk4_advance_probe(double M, double a, double r_obs, double lambda_max, double h_max, const double *states,
                                    const double *p_phi, const uint8_t *refine, const double *lam, const double *h_retry,
                                    const uint32_t *steps, int64_t n, int precision, int n_iters, double *out_states,
                                    double *out_misc, int32_t *out_int)
{
    int rc = require_device();
    if (rc) return rc;
    if (precision != 32 && precision != 64) return fail(LT_ERR_INVALID_ARG, "precision must be 32 or 64");
    if (n <= 0) return LT_OK;
    if (n_iters < 1) return fail(LT_ERR_INVALID_ARG, "n_iters must be at least 1");
    if (!(h_max > 0.0)) return fail(LT_ERR_INVALID_ARG, "h_max must be positive");
    if (!states || !p_phi || !refine || !out_states || !out_misc || !out_int) return fail(LT_ERR_INVALID_ARG, "null pointer");
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    MetricConsts mc;
    if ((rc = make_metric(&m, r_obs, M_PI / 2, 0.0, &mc))) return rc;
    DevBuf ds, dp, dr, dl, dh, dst, os, om, oi;
    if ((rc = probe_upload(ds, states, n * 40)) || (rc = probe_upload(dp, p_phi, n * 8)) || (rc = probe_upload(dr, refine, n)) ||
        (rc = probe_upload(dl, lam, n * 8)) || (rc = probe_upload(dh, h_retry, n * 8)) || (rc = probe_upload(dst, steps, n * 4)) ||
        (rc = os.alloc(n * 40)) || (rc = om.alloc(n * 16)) || (rc = oi.alloc(n * 12))) return rc;
    with_precision(precision, [&](auto t) {
        using T = decltype(t);
        k_rk4_advance_probe<T><<<(unsigned)((n + 63) / 64), 64>>>(make_kerr<T>(mc, lambda_max, h_max), (const double *)ds.p, (const double *)dp.p,
                                                                  (const uint8_t *)dr.p, (const double *)dl.p, (const double *)dh.p,
                                                                  (const uint32_t *)dst.p, n, n_iters, (double *)os.p, (double *)om.p,
                                                                  (int32_t *)oi.p);
    });
    HIP_TRY(hipGetLastError());
    if ((rc = probe_download(out_states, os, n * 40)) || (rc = probe_download(out_misc, om, n * 16)) ||
        (rc = probe_download(out_int, oi, n * 12))) return rc;
    return LT_OK;
}

extern "C" int lt_schw_trace_probe(double M, double r_obs, double phi_max, double h_max, const double *u0, const double *w0,
                                   int64_t n, int precision, double *out, int32_t *out_int, uint32_t *out_n_full, double *out_h_last)
{
    int rc;
    if (precision != 32 && precision != 64) return fail(LT_ERR_INVALID_ARG, "precision must be 32 or 64");
    if (!(phi_max > 0.0) || !(h_max > 0.0) || !(phi_max / h_max <= (double)SCHW_MAX_STEPS))
        return fail(LT_ERR_INVALID_ARG, "phi_max and h_max must be positive, phi_max / h_max at most %u", SCHW_MAX_STEPS);
    lt_metric m{LT_METRIC_SCHWARZSCHILD, 0, M, 0.0};
    MetricConsts mc;
    if ((rc = make_metric(&m, r_obs, M_PI / 2, h_max, &mc))) return rc;
    const SchwConsts<double> plan = make_schw<double>(mc, phi_max, h_max);
    if (out_n_full) *out_n_full = plan.n_full;
    if (out_h_last) *out_h_last = plan.h_last;
    if (n <= 0) return LT_OK; // (the plan is the host's: no device is needed for it)
    if ((rc = require_device())) return rc;
    if (!u0 || !w0 || !out || !out_int) return fail(LT_ERR_INVALID_ARG, "null pointer");
    DevBuf du, dw, dout, di;
    if ((rc = probe_upload(du, u0, n * 8)) || (rc = probe_upload(dw, w0, n * 8)) || (rc = dout.alloc(n * 24)) || (rc = di.alloc(n * 12)))
        return rc;
    with_precision(precision, [&](auto t) {
        using T = decltype(t);
        k_schw_trace_probe<T><<<(unsigned)((n + 255) / 256), 256>>>(make_schw<T>(mc, phi_max, h_max), (const double *)du.p, (const double *)dw.p,
                                                                    n, (double *)dout.p, (int32_t *)di.p);
    });
    HIP_TRY(hipGetLastError());
    if ((rc = probe_download(out, dout, n * 24)) || (rc = probe_download(out_int, di, n * 12))) return rc;
    return LT_OK;
}

extern "C" int lt_extract_probe(int kind, double M, double a, double h_schw, int integrator, const double *fin0, const double *fin1,
                                int64_t n, int precision, double *out_fa, int64_t *out_w, int8_t *out_status, uint32_t *out_evals)
{
    int rc = require_device();
    if (rc) return rc;
    if (precision != 32 && precision != 64) return fail(LT_ERR_INVALID_ARG, "precision must be 32 or 64");
    if (n <= 0) return LT_OK;
    if (!fin0 || !fin1 || !out_fa || !out_w || !out_status || !out_evals) return fail(LT_ERR_INVALID_ARG, "null pointer");
    lt_metric m{kind, 0, M, a};
    MetricConsts mc;
    if ((rc = make_metric(&m, 50.0, M_PI / 2, h_schw, &mc))) return rc;
    count_evals(integrator, &mc);
    DevBuf d0, d1, dfa, dw, dst, dev;
    if ((rc = with_precision(precision, [&](auto t) { return probe_upload_recs<decltype(t)>(d0, fin0, n); })) ||
        (rc = with_precision(precision, [&](auto t) { return probe_upload_recs<decltype(t)>(d1, fin1, n); })) ||
        (rc = dfa.alloc(n * 8)) || (rc = dw.alloc(n * 8)) || (rc = dst.alloc(n)) || (rc = dev.alloc(n * 4))) return rc;
    with_precision(precision, [&](auto t) {
        using T = decltype(t);
        using V = typename Vec4<T>::type;
        k_epilogue_arrays<T><<<(unsigned)((n + 255) / 256), 256>>>(mc, (const V *)d0.p, (const V *)d1.p, n, (double *)dfa.p, (int64_t *)dw.p,
                                                                   (int8_t *)dst.p, (uint32_t *)dev.p);
    });
    HIP_TRY(hipGetLastError());
    if ((rc = probe_download(out_fa, dfa, n * 8)) || (rc = probe_download(out_w, dw, n * 8)) || (rc = probe_download(out_status, dst, n)) ||
        (rc = probe_download(out_evals, dev, n * 4))) return rc;
    return LT_OK;
}

extern "C" int lt_math32_probe(int which, uint32_t bits_lo, uint32_t bits_hi, const float *bases, int n_bases, uint64_t *out)
{
    int rc = require_device();
    if (rc) return rc;
    if (!out || which < 0 || which > 4 || bits_hi < bits_lo || bits_hi - bits_lo >= (1u << 30))
        return fail(LT_ERR_INVALID_ARG, "bad math probe arguments");
    if (which == 3 && (!bases || n_bases < 1 || n_bases > 16)) return fail(LT_ERR_INVALID_ARG, "the shift probe takes 1 to 16 base angles");
    const uint32_t n = bits_hi - bits_lo + 1;
    DevBuf d, db;
    if ((rc = d.alloc(MATH32_OUT * sizeof(uint64_t))) || (rc = db.alloc(16 * sizeof(float)))) return rc;
    uint64_t init[MATH32_OUT] = {0};
    for (int m = 0; m < MATH32_MEASURES; ++m) init[2 + 2 * m] = ~0ull;
    HIP_TRY(hipMemcpy(d.p, init, sizeof(init), hipMemcpyHostToDevice));
    if (which == 3) HIP_TRY(hipMemcpy(db.p, bases, n_bases * sizeof(float), hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)(((uint64_t)n + 256u * MATH32_ITEMS - 1) / (256u * MATH32_ITEMS));
    for (int pass = 0; pass < 2; ++pass) {
        unsigned long long *o = (unsigned long long *)d.p;
        const float *b = (const float *)db.p;
        if (which == 0) k_math32_probe<0><<<grid, 256>>>(bits_lo, n, b, 0, pass, o);
        else if (which == 1) k_math32_probe<1><<<grid, 256>>>(bits_lo, n, b, 0, pass, o);
        else if (which == 2) k_math32_probe<2><<<grid, 256>>>(bits_lo, n, b, 0, pass, o);
        else if (which == 3) k_math32_probe<3><<<grid, 256>>>(bits_lo, n, b, n_bases, pass, o);
        else k_math32_probe<4><<<grid, 256>>>(bits_lo, n, b, 0, pass, o);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpy(out, d.p, sizeof(init), hipMemcpyDeviceToHost));
    return LT_OK;
}

// The float64 primitives, values in and values out; out as in lt_math64_probe.
__global__ void k_math64_probe(int which, const double *__restrict__ x, int64_t n, double *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double u = 0.0, v = 0.0;
    if (which == 0) sincos_f64(x[i], u, v);
    else if (which == 1) M<double>::sincos_small(x[i], u, v);
    else if (which == 2) u = M<double>::rcp_pos(x[i]);
    else if (which == 3) u = pow_m02(x[i]);
    else if (which == 5) u = pow_minus_tenth((float)x[i]);
    else if (which == 6) sincos_f64_exact(x[i], u, v);
    else {
        float s, c;
        M<float>::sincos((float)x[i], s, c);
        u = s; v = c;
    }
    out[i * 2 + 0] = u; out[i * 2 + 1] = v;
}

extern "C" int lt_math64_probe(int which, const double *x, int64_t n, double *out)
{
    int rc = require_device();
    if (rc) return rc;
    if (which < 0 || which > 6) return fail(LT_ERR_INVALID_ARG, "bad math probe arguments");
    if (n <= 0) return LT_OK;
    if (!x || !out) return fail(LT_ERR_INVALID_ARG, "null pointer");
    DevBuf dx, dout;
    if ((rc = dx.alloc(n * 8)) || (rc = dout.alloc(n * 16))) return rc;
    HIP_TRY(hipMemcpy(dx.p, x, n * 8, hipMemcpyHostToDevice));
    k_math64_probe<<<(unsigned)((n + 255) / 256), 256>>>(which, (const double *)dx.p, n, (double *)dout.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.p, n * 16, hipMemcpyDeviceToHost));
    return LT_OK;
}

extern "C" int lt_scatter_rows_dev(const void *d_part, void *d_full, int32_t height, int32_t width, int32_t elem_bytes,
                                   int32_t row_block, int32_t n_parts, int32_t part, void *stream)
{
    int rc = require_device();
    if (rc) return rc;
    int64_t rows = lt_local_rows(height, row_block, n_parts, part);
    if (rows < 0 || width <= 0 || elem_bytes <= 0) return fail(LT_ERR_INVALID_ARG, "bad scatter arguments");
    if (rows > 65535) return fail(LT_ERR_INVALID_ARG, "a partition of %lld rows (at most 65535: grid.y carries the row)", (long long)rows);
    if (rows == 0) return LT_OK;
    if (!d_part || !d_full) return fail(LT_ERR_INVALID_ARG, "null pointer");
    int64_t row_bytes = (int64_t)width * elem_bytes;
    dim3 grid((unsigned)((row_bytes + 16 * 256 - 1) / (16 * 256)), (unsigned)rows);
    k_scatter_rows<<<grid, 256, 0, (hipStream_t)stream>>>((const uint8_t *)d_part, (uint8_t *)d_full, (int)rows, row_bytes,
                                                          row_block, n_parts, part);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_scatter_rows_indexed_dev(const void *d_rows, void *d_full, const int64_t *d_row_index, int64_t n_rows,
                                           int64_t height, int64_t row_bytes, void *stream)
{
    int rc = require_device();
    if (rc) return rc;
    if (n_rows < 0 || height <= 0 || row_bytes <= 0 || n_rows > 65535 * (int64_t)65535)
        return fail(LT_ERR_INVALID_ARG, "bad scatter arguments (n_rows %lld, height %lld, row_bytes %lld)", (long long)n_rows,
                    (long long)height, (long long)row_bytes);
    if (n_rows == 0) return LT_OK;
    if (!d_rows || !d_full || !d_row_index) return fail(LT_ERR_INVALID_ARG, "null pointer");
    // grid.y carries the row (at most 65535 per launch): a frame of more rows goes in slices
    for (int64_t r0 = 0; r0 < n_rows; r0 += 65535) {
        int64_t nr = n_rows - r0 < 65535 ? n_rows - r0 : 65535;
        dim3 grid((unsigned)((row_bytes + 16 * 256 - 1) / (16 * 256)), (unsigned)nr);
        k_scatter_rows_indexed<<<grid, 256, 0, (hipStream_t)stream>>>((const uint8_t *)d_rows + r0 * row_bytes, (uint8_t *)d_full,
                                                                      d_row_index + r0, nr, height, row_bytes);
    }
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

#ifdef LT_PROBES
#include "lt_api_probes.inc"
#endif // LT_PROBES

#include "lt_api_stages.inc"
#include "lt_api_dense.inc"
#include "lt_api_disk.inc"
#include "lt_api_disk_images.inc"
#include "lt_api_hotspot.inc"
#include "lt_api_polarization.inc"
#include "lt_api_hotspot_aa.inc"
#include "lt_api_diskmap.inc"
#include "lt_api_aa.inc"
#include "lt_api_aa_adaptive.inc"
#include "lt_api_spectrum.inc"
#include "lt_api_visibility.inc"
#include "lt_api_visibility_stokes.inc"
#include "lt_api_diskmovie.inc"
#include "lt_api_thermal.inc"
#include "lt_api_thermal_stokes.inc"
#include "lt_api_transfer.inc"
