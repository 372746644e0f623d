// The extractor handle of liborbx's C ABI (include/orbx.h): one plan and one set of device tables per image
// size (planned by orbx_plan.hpp, then by the kernels' own planners), the workspace buffers, launch sequencing
// and the two stereo calls that read the handle's pyramids.  Host code; the kernels are in orbx_pyramid.hip /
// orbx_fast.hip / orbx_quadtree.hip / orbx_describe.hip / orbx_stereo.hip.  Every other entry point sits at
// the end of the .hip that holds its kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/orbx.h"
#include "orbx_host.hpp"
#include "orbx_kernels.hpp"
#include "orbx_plan.hpp"

using namespace orbx;

static_assert(sizeof(Tap) == sizeof(int2) && offsetof(Tap, x) == offsetof(int2, x) &&
                  offsetof(Tap, y) == offsetof(int2, y),
              "the planner's resize tables are uploaded as the kernels' int2 tables");

namespace {

// A buffer that only grows, and whose outgrown block is retired until orbx_destroy rather than freed:
// hipFree / hipHostFree wait for the whole device, which would stall every other stream of the
// process (the other extractor and matcher threads).  Device memory, or pinned host memory.
template <class T, bool Pinned = false>
struct DevBuf {
    T* p = nullptr;
    size_t bytes = 0;
    // p holds at least `count` T afterwards (contents not kept); grows geometrically
    bool reserve(orbx_handle* h, size_t count);
};

// Every size seen keeps its own immutable device tables: a size switch selects another block
// instead of rewriting the tables that kernels of an earlier call (still queued on the caller's
// stream) are reading.  Bounded by the number of distinct image sizes.
struct GeomBlock {
    FramePlan plan;   // geom and cells; the resize tables are dropped once they are uploaded
    GeomTabs dev{};
};

// a block's five device tables with their host data (bands: pyr_plan's, which the block does not keep)
struct Table {
    void** dev;
    const void* host;
    size_t bytes;
};
std::array<Table, 5> tables(GeomBlock& b, const std::vector<int4>& bands = {})
{
    const FramePlan& p = b.plan;
    return {{{(void**)&b.dev.geom, &p.geom, sizeof(Geometry)},
             {(void**)&b.dev.cells, p.cells.data(), sizeof(Cell) * p.cells.size()},
             {(void**)&b.dev.xtab, p.xtab.data(), sizeof(Tap) * p.xtab.size()},
             {(void**)&b.dev.ytab, p.ytab.data(), sizeof(Tap) * p.ytab.size()},
             {(void**)&b.dev.pyr_bands, bands.data(), sizeof(int4) * bands.size()}}};
}

void release(GeomBlock& b)
{
    for (const Table& t : tables(b)) {
        if (*t.dev) (void)hipFree(*t.dev);
        *t.dev = nullptr;
    }
}

}  // namespace

struct orbx_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    orbx_params params{};
    Tables tab;

    // geometry: one block per rows x cols seen (a deque, so that `cur` stays valid), and the selected one
    std::deque<GeomBlock> geom_blocks;
    const GeomBlock* cur = nullptr;
    const Geometry& geom() const { return cur->plan.geom; }
    bool has_size(int rows, int cols) const { return cur && geom().rows == rows && geom().cols == cols; }

    // batch workspace, sized for batch_cap frames of the current geometry; `bufs` is what the launchers take:
    // its geometry tables follow `cur`, its workspace pointers these buffers, its modes orbx_set_cv_modes
    int batch_cap = 0;
    DevBuf<uint8_t> pyr, qt_nodes;
    DevBuf<uint32_t> slots, spill, spill_node, qt_out;
    DevBuf<int> cell_counts, qt_cnt, status;
    ExtractBufs bufs{};

    // host-image path
    DevBuf<uint8_t> img;
    DevBuf<uint8_t> out;   // [keypoints ocap (64-byte rounded)][descriptors ocap x 32], one D2H copy
    DevBuf<uint8_t, true> pin;   // pinned staging: image in, count + keypoints + descriptors out
    int* h_status = nullptr;     // pinned status word (a pageable D2H copy can stall on other streams' work)
    // the host path's stream work (H2D image, the extraction kernels, D2H results and status) as one
    // captured hipGraph, replayed while the buffers and sizes it was captured with stay the same
    struct GraphKey {
        ExtractBufs bufs;
        const void *pin, *img, *out, *pyr;
        long long rows, cols, ocap;
    };
    static_assert(std::has_unique_object_representations_v<GraphKey>, "graph keys are compared as bytes");
    hipGraphExec_t host_graph = nullptr;
    GraphKey graph_key{};
    bool graph_failed = false;

    // The handle's device work is ordered across streams: its workspace (pyramid, candidate slots,
    // quadtree buffers) is shared by every call, so a call on another stream than the last one waits
    // for that call's completion event first (a host extract while a batch is still queued on the
    // caller's stream, or batches of one handle on alternating streams).
    hipEvent_t done_ev = nullptr;
    hipStream_t done_stream = nullptr;
    bool done_pending = false;

    // last batch (for pyramid / debug readback)
    FramePtrs last{};
    int last_batch = 0;
    std::vector<std::vector<uint8_t>> h_levels;
    std::vector<bool> level_cached;

    // timing: one set of 5 events per timed extract call (stage boundaries)
    bool timing = false;
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
    // stage-split extractions (orbx_extract_stage_device): one (start, end) event pair per timed stage
    // call, on that stage's own stream
    std::vector<hipEvent_t> sev;
    std::vector<int> sev_stage;
    int sev_used = 0;

    std::vector<void*> retired_dev, retired_pin;   // outgrown blocks (DevBuf), freed by orbx_destroy
};

namespace {

template <class T, bool Pinned>
bool DevBuf<T, Pinned>::reserve(orbx_handle* h, size_t count)
{
    const size_t need = sizeof(T) * (count ? count : 1);
    if (p && bytes >= need) return true;
    if (p) (Pinned ? h->retired_pin : h->retired_dev).push_back((void*)p);
    const size_t want = std::max(need, bytes + bytes / 2);
    p = nullptr;
    bytes = 0;
    const hipError_t e = Pinned ? hipHostMalloc((void**)&p, want, hipHostMallocDefault) : hipMalloc((void**)&p, want);
    if (e != hipSuccess) {
        p = nullptr;
        return false;
    }
    bytes = want;
    return true;
}

// The handle's own stream serves the synchronous host paths only.  It is created on
// first use: device-batch users bring their own streams, and every idle stream would
// still take one of the process's few hardware queues (GPU_MAX_HW_QUEUES).  HIP maps streams
// onto those queues round-robin, and streams that share a queue run in order, so a host call
// could wait behind an unrelated kernel of the application's.  High-priority streams get
// queues of their own, apart from the application's default-priority streams (measured:
// tests/test_gpu_threads.py); the host matchers' streams are high-priority too (orbx_host.hip).
hipStream_t own_stream(orbx_handle* h)
{
    if (!h->stream) {
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) hi = 0;
        hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, hi);
    }
    return h->stream;
}

void select_geometry(orbx_handle* h, const GeomBlock& b)
{
    h->cur = &b;
    static_cast<GeomTabs&>(h->bufs) = b.dev;
    h->batch_cap = 0;   // re-size the workspace for this geometry (buffers only grow)
}

orbx_status ensure_geometry(orbx_handle* h, int rows, int cols)
{
    if (h->has_size(rows, cols)) return ORBX_OK;
    for (const GeomBlock& b : h->geom_blocks)
        if (b.plan.geom.rows == rows && b.plan.geom.cols == cols) {
            select_geometry(h, b);
            return ORBX_OK;
        }
    GeomBlock b;
    const orbx_status st = plan_frame(h->tab, h->params.ini_th_fast, h->params.min_th_fast, rows, cols, b.plan);
    if (st != ORBX_OK) return st;
    // the kernels' own planners
    Geometry& g = b.plan.geom;
    for (int l = 1; l < g.nlevels; ++l)   // a per-level pyramid launch stages its source rows in one workgroup's LDS
        if (pyr_level_lds(g, l) > 160 * 1024) return ORBX_EINVAL;
    std::vector<int4> pyrbt;
    if (!pyr_plan(g, b.plan.ytab.data(), pyrbt)) return ORBX_EINVAL;
    fast_groups(g);
    // node lists too large for a workgroup's LDS run from global memory (any budget the reference takes)
    if (!qt_prepare(g)) return ORBX_EINVAL;
    int spill = 0;
    for (int l = 0; l < g.nlevels; ++l) spill += std::max(0, g.lv[l].slot_cap - qt_regcap(g, l));
    g.spill_per_frame = std::max(spill, 1);

    // once per image size, into fresh buffers that nothing queued can be reading
    const auto tabs = tables(b, pyrbt);
    for (const Table& t : tabs)
        if (hipMalloc(t.dev, t.bytes ? t.bytes : 16) != hipSuccess) {
            *t.dev = nullptr;
            release(b);
            return ORBX_ENOMEM;
        }
    // on a pooled host-call stream (high priority, orbx_host.hip), so that a handle used only through
    // orbx_extract_batch_device never creates a stream of its own (each takes one of the process's
    // few hardware queues); the copies are complete before any later launch on any stream
    {
        HostCall c(h->device);
        hipStream_t s = c.stream();
        if (s)
            for (const Table& t : tabs)
                if (t.bytes) hipMemcpyAsync(*t.dev, t.host, t.bytes, hipMemcpyHostToDevice, s);
        if (!s || hipStreamSynchronize(s) != hipSuccess) {
            release(b);
            return ORBX_EDEVICE;
        }
    }
    b.plan.xtab = {};
    b.plan.ytab = {};
    h->geom_blocks.push_back(std::move(b));
    select_geometry(h, h->geom_blocks.back());
    return ORBX_OK;
}

orbx_status ensure_batch(orbx_handle* h, int batch)
{
    if (batch <= h->batch_cap) return ORBX_OK;
    const Geometry& g = h->geom();
    ExtractBufs& b = h->bufs;
    const size_t B = (size_t)batch;
    // buf holds count elements afterwards; dst: the launchers' pointer to it
    auto ws = [&](auto& buf, auto*& dst, size_t count) {
        const bool ok = buf.reserve(h, count);
        dst = buf.p;
        return ok;
    };
    if (!h->pyr.reserve(h, (size_t)g.pyr_bytes * B) || !ws(h->slots, b.slots, (size_t)g.slots_per_frame * B) ||
        !ws(h->cell_counts, b.cell_counts, (size_t)g.ncells * B) ||
        !ws(h->spill, b.spill, (size_t)g.spill_per_frame * B) ||
        !ws(h->spill_node, b.spill_node, (size_t)g.spill_per_frame * B) ||
        !ws(h->qt_out, b.qt_out, (size_t)g.out_per_frame * B) || !ws(h->qt_cnt, b.qt_cnt, (size_t)g.nlevels * B) ||
        !ws(h->status, b.status, 16) || !ws(h->qt_nodes, b.qt_nodes, (size_t)g.qtg_per_frame * B)) {
        h->batch_cap = 0;
        return ORBX_ENOMEM;
    }
    h->batch_cap = batch;
    return ORBX_OK;
}

// stream s waits for the handle's last device call when that call was queued on another stream
void order_after_last(orbx_handle* h, hipStream_t s)
{
    if (h->done_pending && h->done_stream != s) hipStreamWaitEvent(s, h->done_ev, 0);
}

// the handle's latest device work is the work queued so far on s
void mark_last(orbx_handle* h, hipStream_t s)
{
    if (!h->done_ev && hipEventCreateWithFlags(&h->done_ev, hipEventDisableTiming) != hipSuccess) {
        h->done_ev = nullptr;
        return;
    }
    hipEventRecord(h->done_ev, s);
    h->done_stream = s;
    h->done_pending = true;
}

// the next set of `per` events of a timed handle's pool (orbx_set_timing), which grows by 64 sets
hipEvent_t* next_events(std::vector<hipEvent_t>& pool, int& used, int per)
{
    if ((size_t)(used + 1) * per > pool.size()) {
        const size_t old = pool.size();
        pool.resize(old + (size_t)per * 64);
        for (size_t i = old; i < pool.size(); ++i) hipEventCreate(&pool[i]);
    }
    return &pool[(size_t)(used++) * per];
}

// the 5 stage-boundary events of one timed extract call
const hipEvent_t* next_stage_events(orbx_handle* h) { return next_events(h->ev, h->ev_used, 5); }

// P is what the handle's last run read and wrote (orbx_get_level, the debug readbacks, the stereo calls)
void note_run(orbx_handle* h, const FramePtrs& P, int batch)
{
    h->last = P;
    h->last_batch = batch;
    std::fill(h->level_cached.begin(), h->level_cached.end(), false);
}

// the extraction's stream work alone (no host state): also what the host path's graph captures;
// ev (timed handles): events recorded at the 5 stage boundaries
void enqueue_pipeline(orbx_handle* h, const FramePtrs& P, int batch, orbx_keypoint* kps, uint8_t* desc, int* counts,
                      int cap, hipStream_t s, const hipEvent_t* ev = nullptr)
{
    const Geometry& g = h->geom();
    const ExtractBufs& b = h->bufs;
    if (counts == h->status.p + 1 && batch == 1) {   // the host path: status and count in one memset
        hipMemsetAsync(h->status.p, 0, 2 * sizeof(int), s);
    } else {
        hipMemsetAsync(counts, 0, sizeof(int) * batch, s);
        hipMemsetAsync(h->status.p, 0, sizeof(int), s);
    }
    if (ev) hipEventRecord(ev[0], s);
    launch_pyramid(g, b, P, batch, s);
    if (ev) hipEventRecord(ev[1], s);
    launch_fast(g, b, P, batch, s);
    if (ev) hipEventRecord(ev[2], s);
    launch_quadtree(g, b, counts, batch, s);
    if (ev) hipEventRecord(ev[3], s);
    launch_describe(g, b, P, kps, desc, cap, batch, s);
    if (ev) hipEventRecord(ev[4], s);
}

orbx_status run_pipeline(orbx_handle* h, const FramePtrs& P, int batch, orbx_keypoint* kps, uint8_t* desc,
                         int* counts, int cap, hipStream_t s)
{
    enqueue_pipeline(h, P, batch, kps, desc, counts, cap, s, h->timing ? next_stage_events(h) : nullptr);
    note_run(h, P, batch);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

bool ensure_status_word(orbx_handle* h)
{
    if (!h->h_status && hipHostMalloc((void**)&h->h_status, 64, hipHostMallocDefault) != hipSuccess) {
        h->h_status = nullptr;
        return false;
    }
    return true;
}

orbx_status status_from_device(orbx_handle* h, hipStream_t s)
{
    if (!ensure_status_word(h)) return ORBX_ENOMEM;
    if (hipMemcpyAsync(h->h_status, h->status.p, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess)
        return ORBX_EDEVICE;
    if (hipStreamSynchronize(s) != hipSuccess) return ORBX_EDEVICE;
    const int st = *h->h_status;
    if (st & kStatusCapOverflow) return ORBX_ENOSPC;
    if (st) return ORBX_EDEVICE;
    return ORBX_OK;
}

}  // namespace

extern "C" {

orbx_status orbx_create(const orbx_params* params, int device, orbx_handle** out)
{
    if (!params || !out) return ORBX_EINVAL;
    *out = nullptr;
    orbx_handle* h = new (std::nothrow) orbx_handle();
    if (!h) return ORBX_ENOMEM;
    h->params = *params;
    if (!make_tables(*params, h->tab)) {
        delete h;
        return ORBX_EINVAL;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        delete h;
        return ORBX_EDEVICE;
    }
    h->device = device;
    h->h_levels.resize(kMaxLevels);
    h->level_cached.assign(kMaxLevels, false);
    *out = h;
    return ORBX_OK;
}

void orbx_destroy(orbx_handle* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->pin.p) hipHostFree(h->pin.p);
    if (h->h_status) hipHostFree(h->h_status);
    for (void* p : h->retired_pin) hipHostFree(p);
    for (void* p : h->retired_dev) (void)hipFree(p);
    for (GeomBlock& b : h->geom_blocks) release(b);
    auto drop = [](auto&... b) { ((b.p ? (void)hipFree(b.p) : (void)0), ...); };
    drop(h->pyr, h->slots, h->cell_counts, h->spill, h->spill_node, h->qt_nodes, h->qt_out, h->qt_cnt, h->status,
         h->img, h->out);
    for (auto& e : h->ev)
        if (e) hipEventDestroy(e);
    for (auto& e : h->sev)
        if (e) hipEventDestroy(e);
    if (h->host_graph) hipGraphExecDestroy(h->host_graph);
    if (h->done_ev) hipEventDestroy(h->done_ev);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

orbx_status orbx_set_cv_modes(orbx_handle* h, int resize_mode, int blur_mode)
{
    if (!h || (resize_mode != ORBX_RESIZE_SCALAR && resize_mode != ORBX_RESIZE_SSE2) ||
        (blur_mode != ORBX_BLUR_SCALAR && blur_mode != ORBX_BLUR_SSE2 && blur_mode != ORBX_BLUR_BITEXACT))
        return ORBX_EINVAL;
    h->bufs.resize_mode = resize_mode;
    h->bufs.blur_mode = blur_mode;
    std::fill(h->level_cached.begin(), h->level_cached.end(), false);
    return ORBX_OK;
}

orbx_status orbx_get_tables(const orbx_handle* h, int* nlevels, float* scale_factor, float* scale, float* inv_scale,
                            float* sigma2, float* inv_sigma2, int* features_per_level)
{
    if (!h) return ORBX_EINVAL;
    const Tables& t = h->tab;
    if (nlevels) *nlevels = t.nlevels;
    if (scale_factor) *scale_factor = h->params.scale_factor;
    for (int l = 0; l < t.nlevels; ++l) {
        if (scale) scale[l] = t.scale[l];
        if (inv_scale) inv_scale[l] = t.inv_scale[l];
        if (sigma2) sigma2[l] = t.sigma2[l];
        if (inv_sigma2) inv_sigma2[l] = t.inv_sigma2[l];
        if (features_per_level) features_per_level[l] = t.nfeat[l];
    }
    return ORBX_OK;
}

int orbx_capacity(const orbx_handle* h, int rows, int cols)
{
    if (!h) return -1;
    orbx_handle* m = const_cast<orbx_handle*>(h);
    DeviceGuard guard(m->device);
    if (ensure_geometry(m, rows, cols) != ORBX_OK) return -1;
    return m->geom().out_per_frame;
}

orbx_status orbx_debug_launches(orbx_handle* h, int rows, int cols, int batch, int* counts, int n)
{
    if (!h || !counts || n < 1 || batch < 1) return ORBX_EINVAL;
    DeviceGuard guard(h->device);
    const orbx_status st = ensure_geometry(h, rows, cols);
    if (st != ORBX_OK) return st;
    const Geometry& g = h->geom();
    // the launchers' own plans; the pyramid's launches each read one level (counts[4]: bit mask)
    const PyrLaunches pl = pyr_launches(g, batch);
    FastRun run[kFastMaxRuns];
    QtGroup grp[kQtMaxGroups];
    const int c[5] = {pl.n, fast_plan(g, batch, run), qt_plan(g, batch, grp), 1, pl.srcmask};
    for (int i = 0; i < n; ++i) counts[i] = i < 5 ? c[i] : 0;
    return ORBX_OK;
}

orbx_status orbx_debug_qt_plan(orbx_handle* h, int rows, int cols, int batch, int* plan, int nlevels)
{
    if (!h || !plan || batch < 1) return ORBX_EINVAL;
    DeviceGuard guard(h->device);
    const orbx_status st = ensure_geometry(h, rows, cols);
    if (st != ORBX_OK) return st;
    const Geometry& g = h->geom();
    if (nlevels < g.nlevels) return ORBX_EINVAL;
    static_assert(sizeof(QtLevelPlan) == 8 * sizeof(int), "orbx_debug_qt_plan rows are eight ints");
    qt_report(g, batch, (QtLevelPlan*)plan);
    return ORBX_OK;
}

// Host-path copies between the pinned staging block and device memory as kernels on the extraction's own
// queue: an SDMA copy (hipMemcpy*Async) costs its own ~11 us for a 640x480 image plus ~11 us before the
// compute queue sees it has finished; a kernel reading or writing the mapped pinned block over PCIe needs
// neither.  Two (src, dst, 16-byte units) regions per launch.
__global__ __launch_bounds__(256) void k_host_copy(const uint4* __restrict__ s0, uint4* __restrict__ d0, size_t n0,
                                                   const uint4* __restrict__ s1, uint4* __restrict__ d1, size_t n1)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n0 + n1; i += stride) {
        if (i < n0) d0[i] = s0[i];
        else d1[i - n0] = s1[i - n0];
    }
}

orbx_status orbx_extract(orbx_handle* h, const uint8_t* img, int rows, int cols, size_t step, orbx_keypoint* kps,
                         int cap, uint8_t* desc, int* n_out)
{
    if (!h || !n_out) return ORBX_EINVAL;
    if (!img || rows <= 0 || cols <= 0) return ORBX_EMPTY;   // src/ORBextractor.cc:1252
    if (step < (size_t)cols || !kps || !desc || cap < 0) return ORBX_EINVAL;
    DeviceGuard guard(h->device);
    orbx_status st = ensure_geometry(h, rows, cols);
    if (st != ORBX_OK) return st;
    if ((st = ensure_batch(h, 1)) != ORBX_OK) return st;
    const int pitch = (cols + 63) & ~63;
    const size_t need = (size_t)pitch * rows;
    if (!h->img.reserve(h, need)) return ORBX_ENOMEM;
    const int ocap = h->geom().out_per_frame;
    // device results [keypoints ocap][descriptors ocap x 32] mirror the pinned block from kp_off, and the
    // frame's count sits in the status block's second word: two D2H copies (status + count, results)
    const size_t kp_b = ((size_t)ocap * sizeof(orbx_keypoint) + 63) & ~(size_t)63;
    if (!h->out.reserve(h, kp_b + (size_t)ocap * 32)) return ORBX_ENOMEM;
    // pinned staging: [image rows x pitch][status, count (16 bytes)][keypoints ocap][descriptors ocap x 32]
    const size_t img_b = need;   // pitch * rows, a multiple of 64
    const size_t kp_off = img_b + 64, ds_off = kp_off + kp_b;
    const size_t pin_need = ds_off + (size_t)ocap * 32;
    if (!h->pin.reserve(h, pin_need)) return ORBX_ENOMEM;
    for (int r = 0; r < rows; ++r) std::memcpy(h->pin.p + (size_t)r * pitch, img + (size_t)r * step, (size_t)cols);
    hipStream_t s = own_stream(h);
    order_after_last(h, s);
    FramePtrs P{h->img.p, need, pitch, h->pyr.p, (size_t)h->geom().pyr_bytes};
    int* phdr = (int*)(h->pin.p + img_b);   // [0] status, [1] count
    int* d_count = h->status.p + 1;
    orbx_keypoint* d_kps = (orbx_keypoint*)h->out.p;
    uint8_t* d_desc = h->out.p + kp_b;
    // H2D image, the kernels, then one round trip: status, count and the whole output capacity
    // a timed handle (orbx_set_timing) launches directly, recording the stage events
    const hipEvent_t* ev = h->timing ? next_stage_events(h) : nullptr;
    // the pinned block's device address (the same pointer under unified addressing)
    void* dpin = nullptr;
    if (hipHostGetDevicePointer(&dpin, h->pin.p, 0) != hipSuccess) dpin = nullptr;
    const bool kcopy = dpin != nullptr;   // else SDMA copies
    uint8_t* dp = (uint8_t*)dpin;
    const size_t out_b = kp_b + (size_t)ocap * 32;   // multiple of 32
    auto enqueue = [&]() {
        if (kcopy) {   // the image rows at the device pitch, so the copy is whole 16-byte units
            hipLaunchKernelGGL(k_host_copy, dim3(std::min<size_t>((need / 16 + 255) / 256, 1024)), dim3(256), 0, s,
                               (const uint4*)dp, (uint4*)h->img.p, need / 16, (const uint4*)nullptr, (uint4*)nullptr,
                               (size_t)0);
        } else {
            hipMemcpyAsync(h->img.p, h->pin.p, need, hipMemcpyHostToDevice, s);
        }
        enqueue_pipeline(h, P, 1, d_kps, d_desc, d_count, ocap, s, ev);
        if (kcopy) {   // status + count (the status block's first 16 bytes) and the whole output capacity
            hipLaunchKernelGGL(k_host_copy, dim3(std::min<size_t>((out_b / 16 + 1 + 255) / 256, 1024)), dim3(256), 0, s,
                               (const uint4*)h->status.p, (uint4*)(dp + img_b), (size_t)1, (const uint4*)h->out.p,
                               (uint4*)(dp + kp_off), out_b / 16);
        } else {
            hipMemcpyAsync(phdr, h->status.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s);
            hipMemcpyAsync(h->pin.p + kp_off, h->out.p, out_b, hipMemcpyDeviceToHost, s);
        }
    };
    // Replayed as a hipGraph: one submission instead of ~17 (launch overhead is most of a 640x480 frame's
    // latency).  The graph is re-captured when any buffer or size it holds changes.
    const orbx_handle::GraphKey key{h->bufs, h->pin.p, h->img.p, h->out.p, h->pyr.p, rows, cols, ocap};
    bool launched = false;
    if (!ev && !h->graph_failed && !getenv("ORBX_NO_GRAPH")) {
        if (h->host_graph && std::memcmp(&h->graph_key, &key, sizeof key)) {
            hipGraphExecDestroy(h->host_graph);
            h->host_graph = nullptr;
        }
        if (!h->host_graph) {
            hipGraph_t graph = nullptr;
            bool ok = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess;
            if (ok) {
                enqueue();
                ok = hipStreamEndCapture(s, &graph) == hipSuccess && graph;
            }
            ok = ok && hipGraphInstantiate(&h->host_graph, graph, nullptr, nullptr, 0) == hipSuccess;
            if (graph) hipGraphDestroy(graph);
            if (!ok) {
                (void)hipGetLastError();
                h->host_graph = nullptr;
                h->graph_failed = true;   // direct launches from now on
            }
            h->graph_key = key;
        }
        launched = h->host_graph && hipGraphLaunch(h->host_graph, s) == hipSuccess;
    }
    if (!launched) enqueue();
    if (hipGetLastError() != hipSuccess) return ORBX_EDEVICE;
    note_run(h, P, 1);
    if (hipStreamSynchronize(s) != hipSuccess) return ORBX_EDEVICE;
    h->done_pending = false;   // everything the handle queued has completed
    if (phdr[0] & kStatusCapOverflow) return ORBX_ENOSPC;
    if (phdr[0]) return ORBX_EDEVICE;
    const int n = phdr[1];
    if (n > cap) return ORBX_ENOSPC;
    if (n > 0) {
        std::memcpy(kps, h->pin.p + kp_off, sizeof(orbx_keypoint) * (size_t)n);
        std::memcpy(desc, h->pin.p + ds_off, (size_t)n * 32);
    }
    *n_out = n;
    return ORBX_OK;
}

orbx_status orbx_get_level(orbx_handle* h, int level, const uint8_t** data, int* rows, int* cols, size_t* step)
{
    if (!h || !h->cur || h->last_batch <= 0 || level < 0 || level >= h->geom().nlevels) return ORBX_EINVAL;
    DeviceGuard guard(h->device);
    const LevelGeom& L = h->geom().lv[level];
    if (!h->level_cached[level]) {
        std::vector<uint8_t>& v = h->h_levels[level];
        v.resize((size_t)L.w * L.h);
        const uint8_t* src;
        size_t sp;
        if (level == 0) {
            src = h->last.in;
            sp = (size_t)h->last.in_pitch;
        } else {
            src = h->last.pyr + L.pyr_off;
            sp = (size_t)L.pitch;
        }
        order_after_last(h, own_stream(h));
        if (hipMemcpy2DAsync(v.data(), L.w, src, sp, L.w, L.h, hipMemcpyDeviceToHost, own_stream(h)) != hipSuccess ||
            hipStreamSynchronize(own_stream(h)) != hipSuccess)
            return ORBX_EDEVICE;
        h->level_cached[level] = true;
    }
    if (data) *data = h->h_levels[level].data();
    if (rows) *rows = L.h;
    if (cols) *cols = L.w;
    if (step) *step = (size_t)L.w;
    return ORBX_OK;
}

orbx_status orbx_extract_batch_device(orbx_handle* h, const uint8_t* d_imgs, int batch, int rows, int cols,
                                      size_t step, size_t frame_stride, orbx_keypoint* d_kps, uint8_t* d_desc,
                                      int* d_counts, int cap, void* stream)
{
    if (!h || !d_imgs || batch <= 0 || !d_kps || !d_desc || !d_counts || cap <= 0) return ORBX_EINVAL;
    if (step < (size_t)cols || (batch > 1 && frame_stride < step * (size_t)rows)) return ORBX_EINVAL;
    DeviceGuard guard(h->device);
    orbx_status st = ensure_geometry(h, rows, cols);
    if (st != ORBX_OK) return st;
    if ((st = ensure_batch(h, batch)) != ORBX_OK) return st;
    hipStream_t s = (hipStream_t)stream;   // taken literally: NULL is the HIP null stream
    order_after_last(h, s);
    FramePtrs P{d_imgs, frame_stride, (int)step, h->pyr.p, (size_t)h->geom().pyr_bytes};
    st = run_pipeline(h, P, batch, d_kps, d_desc, d_counts, cap, s);
    mark_last(h, s);
    return st;
}

orbx_status orbx_extract_stage_device(orbx_handle* h, int stage, const uint8_t* d_imgs, int batch, int rows, int cols,
                                      size_t step, size_t frame_stride, orbx_keypoint* d_kps, uint8_t* d_desc,
                                      int* d_counts, int cap, void* stream)
{
    if (!h || stage < 0 || stage > 3 || !d_imgs || batch <= 0 || !d_kps || !d_desc || !d_counts || cap <= 0)
        return ORBX_EINVAL;
    if (step < (size_t)cols || (batch > 1 && frame_stride < step * (size_t)rows)) return ORBX_EINVAL;
    DeviceGuard guard(h->device);
    orbx_status st;
    if (stage == 0) {   // sizes the geometry and workspace; later stages must match them
        if ((st = ensure_geometry(h, rows, cols)) != ORBX_OK) return st;
        if ((st = ensure_batch(h, batch)) != ORBX_OK) return st;
    } else if (!h->has_size(rows, cols) || batch > h->batch_cap) {
        return ORBX_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const Geometry& g = h->geom();
    const ExtractBufs& b = h->bufs;
    FramePtrs P{d_imgs, frame_stride, (int)step, h->pyr.p, (size_t)g.pyr_bytes};
    hipEvent_t* tev = nullptr;   // a timed handle: this stage's (start, end) events
    if (h->timing) {
        tev = next_events(h->sev, h->sev_used, 2);
        h->sev_stage.resize(h->sev.size() / 2);
        h->sev_stage[h->sev_used - 1] = stage;
    }
    // the previous batch's describe and any stereo search still reading its pyramids (the caller orders
    // the rest); before the start event, so the wait is not counted as pyramid time
    if (stage == 0) order_after_last(h, s);
    if (tev) hipEventRecord(tev[0], s);
    switch (stage) {
    case 0:
        hipMemsetAsync(d_counts, 0, sizeof(int) * batch, s);
        hipMemsetAsync(h->status.p, 0, sizeof(int), s);
        launch_pyramid(g, b, P, batch, s);
        break;
    case 1:
        launch_fast(g, b, P, batch, s);
        break;
    case 2:
        launch_quadtree(g, b, d_counts, batch, s);
        break;
    default:
        launch_describe(g, b, P, d_kps, d_desc, cap, batch, s);
        note_run(h, P, batch);
        mark_last(h, s);
        break;
    }
    if (tev) hipEventRecord(tev[1], s);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbx_sync(orbx_handle* h, void* stream)
{
    if (!h) return ORBX_EINVAL;
    DeviceGuard guard(h->device);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return ORBX_EDEVICE;
    if (!h->status.p) return ORBX_OK;
    return status_from_device(h, (hipStream_t)stream);
}

orbx_status orbx_set_timing(orbx_handle* h, int enable)
{
    if (!h) return ORBX_EINVAL;
    h->timing = enable != 0;
    h->ev_used = 0;   // (re)start accumulation
    h->sev_used = 0;
    return ORBX_OK;
}

orbx_status orbx_get_stage_times(orbx_handle* h, float* ms, int n)
{
    if (!h || !ms || (h->ev_used == 0 && h->sev_used == 0)) return ORBX_EINVAL;
    for (int i = 0; i < n && i < 4; ++i) ms[i] = 0.f;
    for (int c = 0; c < h->sev_used; ++c) {   // stage-split calls (their streams may differ)
        const hipEvent_t* e = &h->sev[(size_t)c * 2];
        float t = 0.f;
        if (hipEventSynchronize(e[1]) != hipSuccess) return ORBX_EDEVICE;
        hipEventElapsedTime(&t, e[0], e[1]);
        if (h->sev_stage[c] < n) ms[h->sev_stage[c]] += t;
    }
    if (h->ev_used > 0 && hipEventSynchronize(h->ev[(size_t)h->ev_used * 5 - 1]) != hipSuccess) return ORBX_EDEVICE;
    for (int c = 0; c < h->ev_used; ++c) {
        const hipEvent_t* e = &h->ev[(size_t)c * 5];
        for (int i = 0; i < n && i < 4; ++i) {
            float t = 0.f;
            hipEventElapsedTime(&t, e[i], e[i + 1]);
            ms[i] += t;
        }
    }
    return ORBX_OK;
}

orbx_status orbx_debug_pyramid(orbx_handle* h, int frame, uint8_t* out, size_t out_size)
{
    if (!h || !out || frame < 0 || frame >= h->last_batch) return ORBX_EINVAL;
    DeviceGuard guard(h->device);
    order_after_last(h, own_stream(h));
    size_t o = 0;
    for (int l = 0; l < h->geom().nlevels; ++l) {
        const LevelGeom& L = h->geom().lv[l];
        if (o + (size_t)L.w * L.h > out_size) return ORBX_ENOSPC;
        const uint8_t* src;
        size_t sp;
        if (l == 0) {
            src = h->last.in + (size_t)frame * h->last.in_fstride;
            sp = (size_t)h->last.in_pitch;
        } else {
            src = h->last.pyr + (size_t)frame * h->last.pyr_fstride + L.pyr_off;
            sp = (size_t)L.pitch;
        }
        hipMemcpy2DAsync(out + o, L.w, src, sp, L.w, L.h, hipMemcpyDeviceToHost, own_stream(h));
        o += (size_t)L.w * L.h;
    }
    return hipStreamSynchronize(own_stream(h)) == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbx_debug_candidates(orbx_handle* h, int frame, int level, int* xys, int cap, int* n)
{
    if (!h || !n || frame < 0 || frame >= h->last_batch || level < 0 || level >= h->geom().nlevels) return ORBX_EINVAL;
    DeviceGuard guard(h->device);
    order_after_last(h, own_stream(h));
    const Geometry& g = h->geom();
    std::vector<int> cnt(g.ncells);
    std::vector<uint32_t> sl(g.slots_per_frame);
    hipMemcpyAsync(cnt.data(), h->cell_counts.p + (size_t)frame * g.ncells, sizeof(int) * g.ncells,
                   hipMemcpyDeviceToHost, own_stream(h));
    hipMemcpyAsync(sl.data(), h->slots.p + (size_t)frame * g.slots_per_frame, sizeof(uint32_t) * g.slots_per_frame,
                   hipMemcpyDeviceToHost, own_stream(h));
    if (hipStreamSynchronize(own_stream(h)) != hipSuccess) return ORBX_EDEVICE;
    const LevelGeom& L = g.lv[level];
    // a cell's first slot: its own slot base if FAST wrote it directly (kCellDirect), else its wave's run
    // (the wave's first cell's slot base plus the wave's earlier cells' counts; orbx_kernels.hpp)
    const int cpw = fast_cells_per_wave(h->last_batch);
    int k = 0;
    uint32_t run = 0;
    for (int c = L.cell_begin; c < L.cell_begin + L.ncells; ++c) {
        const uint32_t raw = (uint32_t)cnt[c];
        const int n = (int)(raw & ~kCellDirect);
        if ((c - L.cell_begin) % cpw == 0) run = (uint32_t)h->cur->plan.cells[c].slot_base;
        const uint32_t a = (raw & kCellDirect) ? (uint32_t)h->cur->plan.cells[c].slot_base : run;
        run += (raw & kCellDirect) ? 0u : (uint32_t)n;
        for (int i = 0; i < n; ++i) {
            const uint32_t v = sl[a + i];
            if (k < cap && xys) {
                xys[3 * k] = (int)kp_x(v, (uint32_t)g.kp_xbits);
                xys[3 * k + 1] = (int)kp_y(v, (uint32_t)g.kp_xbits);
                xys[3 * k + 2] = (int)(v >> 24);
            }
            ++k;
        }
    }
    *n = k;
    return k > cap ? ORBX_ENOSPC : ORBX_OK;
}

orbx_status orbx_debug_fill_workspace(orbx_handle* h, int value)
{
    if (!h) return ORBX_EINVAL;
    DeviceGuard guard(h->device);
    hipStream_t s = own_stream(h);
    order_after_last(h, s);
    const int v = value & 0xFF;
    if (h->pyr.p && hipMemsetAsync(h->pyr.p, v, h->pyr.bytes, s) != hipSuccess) return ORBX_EDEVICE;
    if (h->img.p && hipMemsetAsync(h->img.p, v, h->img.bytes, s) != hipSuccess) return ORBX_EDEVICE;
    if (hipStreamSynchronize(s) != hipSuccess) return ORBX_EDEVICE;
    h->done_pending = false;   // everything the handle queued has completed
    // the staged image is copied whole, row padding included, from the pinned block (orbx_extract): fill the
    // image rows there too, or the next host call would copy the block's old padding over the fill
    if (h->pin.p) std::memset(h->pin.p, v, std::min(h->pin.bytes, h->img.bytes));
    std::fill(h->level_cached.begin(), h->level_cached.end(), false);
    return ORBX_OK;
}

}  // extern "C"

namespace {

// search limits of ComputeStereoMatches (src/Frame.cc:676-681, mb from :140) and the
// row-band half width that bounds every right keypoint's [floor(y-r), ceil(y+r)]
void stereo_limits(const orbx_handle* h, float bf, float fx, float* maxD, int* rband)
{
    const float mb = bf / fx;
    const float minZ = mb;
    *maxD = bf / minZ;
    float rmax = 0.f;
    for (int l = 0; l < h->tab.nlevels; ++l) rmax = std::max(rmax, 2.0f * h->tab.scale[l]);
    *rband = (int)std::ceil(rmax);
}

bool same_geometry(const orbx_handle* a, const orbx_handle* b)
{
    if (!a->cur || !b->cur || !a->has_size(b->geom().rows, b->geom().cols)) return false;
    if (a->tab.nlevels != b->tab.nlevels) return false;
    for (int l = 0; l < a->tab.nlevels; ++l)
        if (a->tab.scale[l] != b->tab.scale[l]) return false;
    return true;
}

}  // namespace

extern "C" {

orbx_status orbx_compute_stereo_matches(orbx_handle* left, orbx_handle* right, const orbx_keypoint* kps_l,
                                        const uint8_t* desc_l, int n_l, const orbx_keypoint* kps_r,
                                        const uint8_t* desc_r, int n_r, float bf, float fx, float* u_right,
                                        float* depth, int* n_good)
{
    if (!left || !right || !n_good || n_l < 0 || n_r < 0) return ORBX_EINVAL;
    *n_good = 0;
    if (n_l == 0) return ORBX_OK;   // Frame ctor returns before ComputeStereoMatches (src/Frame.cc:106-107)
    if (!kps_l || !desc_l || !u_right || !depth || (n_r > 0 && (!kps_r || !desc_r))) return ORBX_EINVAL;
    if (left->device != right->device || !same_geometry(left, right) || left->last_batch <= 0 ||
        right->last_batch <= 0 || !(fx != 0.f) || !(bf != 0.f))
        return ORBX_EINVAL;
    const int cap = std::max(n_l, n_r);
    if (cap > 32767) return ORBX_EINVAL;
    HostCall c(left->device);
    const int hmeta[5] = {n_l, n_r, 0, 1, 0};   // counts[2], fl, fr, ngood
    const auto om = c.in(hmeta, 5);
    // the kernels address frame f's keypoints at kps + f * cap: left rows at 0, right rows at cap
    const auto ok = c.stage<orbx_keypoint>(2 * (size_t)cap);
    const auto od = c.stage<uint8_t>((size_t)64 * cap);
    const auto ou = c.out<float>((size_t)cap), oz = c.out<float>((size_t)cap);
    const auto osad = c.out<int>((size_t)cap);
    orbx_status st = c.prepare();
    if (st != ORBX_OK) return st;
    pack_pair(c.host(ok), (size_t)cap, kps_l, (size_t)n_l, kps_r, (size_t)n_r);
    pack_pair(c.host(od), (size_t)32 * cap, desc_l, (size_t)32 * n_l, desc_r, (size_t)32 * n_r);
    if ((st = c.upload()) != ORBX_OK) return st;
    // the two images' pyramids: written by each handle's last extraction, on whatever stream it ran
    order_after_last(left, c.stream());
    if (right != left) order_after_last(right, c.stream());
    // single images: frame strides 0, so frame indices 0 / 1 both address the handle's image
    FramePtrs PL = left->last, PR = right->last;
    PL.in_fstride = PL.pyr_fstride = 0;
    PR.in_fstride = PR.pyr_fstride = 0;
    float maxD;
    int rband;
    stereo_limits(left, bf, fx, &maxD, &rband);
    launch_stereo(left->geom(), left->bufs.geom, PL, PR, c.dev(ok), c.dev(od), c.dev(om), cap, c.dev(om, 2),
                  c.dev(om, 3), 1, bf, maxD, rband, c.dev(ou), c.dev(oz), c.dev(osad), c.dev(om, 4), c.stream());
    if (hipGetLastError() != hipSuccess) return ORBX_EDEVICE;
    int ng = 0;
    c.fetch(ou, u_right, (size_t)n_l);
    c.fetch(oz, depth, (size_t)n_l);
    c.fetch(om, &ng, 1, 4);
    if ((st = c.finish()) != ORBX_OK) return st;
    *n_good = ng;
    return ORBX_OK;
}

orbx_status orbx_stereo_batch_device(orbx_handle* h, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                     const int* d_counts, int cap, const int* d_left, const int* d_right, int npairs,
                                     float bf, float fx, float* d_u_right, float* d_depth, int* d_n_good,
                                     void* stream)
{
    if (!h || !d_kps || !d_desc || !d_counts || cap <= 0 || cap > 32767 || npairs < 0 || !d_left || !d_right ||
        !d_u_right || !d_depth || !d_n_good || !(fx != 0.f) || !(bf != 0.f))
        return ORBX_EINVAL;
    if (!h->cur || h->last_batch <= 0) return ORBX_EINVAL;
    if (npairs == 0) return ORBX_OK;
    DeviceGuard guard(h->device);
    hipStream_t s = (hipStream_t)stream;
    order_after_last(h, s);   // the batch's pyramids
    int* dsad = nullptr;
    if (hipMallocAsync((void**)&dsad, sizeof(int) * (size_t)npairs * cap, s) != hipSuccess) return ORBX_ENOMEM;
    float maxD;
    int rband;
    stereo_limits(h, bf, fx, &maxD, &rband);
    launch_stereo(h->geom(), h->bufs.geom, h->last, h->last, d_kps, d_desc, d_counts, cap, d_left, d_right, npairs, bf,
                  maxD, rband, d_u_right, d_depth, dsad, d_n_good, s);
    hipFreeAsync(dsad, s);
    // the stereo kernels read the handle's pyramid workspace: the next extraction, which rewrites it, waits
    // for them (s already waited for the extraction, so this event covers both)
    mark_last(h, s);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

}  // extern "C"
