// gsr_shard.cpp -- the multi-GPU step in C++ (see gsr_shard.h): ShardStep with its
// buffer Pool and allocation Arenas, and the per-rank host threads of an in-process group.  The
// transports are gsr_exchange.cpp, the partition arithmetic gsr_plan.cpp, the tensor-to-ABI glue
// gsr_render.h's detail::.
#include "gsr_shard.h"

#include <ATen/hip/HIPGraph.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/StreamGuard.h>

#include <algorithm>
#include <exception>
#include <thread>

namespace gsr {
namespace {

using Stream = c10::hip::HIPStreamMasqueradingAsCUDA;
// c10's device-generic guard and events: no HIP runtime symbol is referenced here (gsr_exchange.cpp)
using StreamGuard = c10::StreamGuard;
using detail::dev_view;

Stream current_stream() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(); }

template <class F>
void run_threads(const std::vector<ShardStep*>& steps, F&& body) {
    std::vector<std::thread> th;
    std::vector<std::exception_ptr> err(steps.size());
    const c10::Device dev(c10::DeviceType::CUDA, c10::hip::current_device());
    for (size_t r = 0; r < steps.size(); ++r)
        th.emplace_back([&, r] {
            try {
                c10::DeviceGuard g(dev);
                body(*steps[r]);
            } catch (...) {
                err[r] = std::current_exception();
            }
        });
    for (auto& t : th) t.join();
    for (auto& e : err)
        if (e) std::rethrow_exception(e);
}

// Fixed-address arena behind one gsr_alloc_fn role: the i-th request of a step gets slot i,
// grown only when a request is larger (never during a captured step: capacities are fixed).
struct Arena {
    torch::Device dev;
    std::vector<torch::Tensor> slots;
    size_t next = 0;
    bool frozen = false;
    static void* cb(void* ctx, size_t bytes) {
        auto* a = static_cast<Arena*>(ctx);
        const size_t i = a->next++;
        if (i == a->slots.size()) {
            if (a->frozen) return nullptr;
            a->slots.push_back(torch::empty({(int64_t)std::max<size_t>(bytes, 16)},
                                            torch::TensorOptions().dtype(torch::kUInt8).device(a->dev)));
        } else if ((size_t)a->slots[i].numel() < bytes) {
            if (a->frozen) return nullptr;
            a->slots[i] = torch::empty({(int64_t)bytes}, torch::TensorOptions().dtype(torch::kUInt8).device(a->dev));
        }
        return a->slots[i].data_ptr();
    }
};

}  // namespace

void run_ranks_plan(const std::vector<ShardStep*>& steps) {
    run_threads(steps, [](ShardStep& s) { s.plan(); });
}
void run_ranks_steps(const std::vector<ShardStep*>& steps, const torch::Tensor& dpix, int n) {
    run_threads(steps, [&](ShardStep& s) {
        for (int i = 0; i < n; ++i) s.step(dpix);
        s.check();
    });
}

ShardOverflowError::ShardOverflowError(int64_t step_, int rank_, std::vector<int64_t> counts_, int pair_cap_,
                                       int64_t band_k_, int capacity_)
    : std::overflow_error([&] {
          std::string s = "multi-GPU step " + std::to_string(step_) + " overflowed on rank " + std::to_string(rank_) +
                          ": splats per band [";
          for (size_t i = 0; i < counts_.size(); ++i) s += (i ? ", " : "") + std::to_string(counts_[i]);
          return s + "] vs pair_cap " + std::to_string(pair_cap_) + ", band instances " + std::to_string(band_k_) +
                 " vs capacity " + std::to_string(capacity_);
      }()),
      step(step_), rank(rank_), counts(std::move(counts_)), pair_cap(pair_cap_), band_k(band_k_),
      capacity(capacity_) {}

// ---- the step ----
// gsr_band_forward takes one ctx for its three allocation roles: ctx = the Pool, one callback
// per role.  Streams, events and the captured graph are libtorch's (no HIP runtime call here).
struct ShardStep::Pool {
    torch::Device dev;
    torch::Tensor send, recv, state, radii, color, g2, back, mine, gathered, image;
    detail::LeafGrads lg;                        // the shard's leaf gradients and their gsr_grads
    std::map<std::string, torch::Tensor> grads;  // the same tensors by name (Result::grads)
    Arena geom{dev}, bin{dev}, img{dev}, scratch{dev};
    gsr_buffers bufs{};
    size_t block_bytes = 0, grad_block = 0, mine_floats = 0, status_off = 0;
    int tall = 0;
    Stream main, side;  // the step's stream (capturable) and the all-gather's
    c10::Event enter{c10::DeviceType::CUDA}, leave{c10::DeviceType::CUDA}, fork{c10::DeviceType::CUDA},
        join{c10::DeviceType::CUDA};
    std::vector<torch::Tensor> ring;  // pinned (world x foot_words) int32 per slot
    std::vector<std::unique_ptr<c10::Event>> ring_ev;
    std::unique_ptr<at::cuda::CUDAGraph> graph;
    const void* graph_dpix = nullptr;
    // capture only once the camera and dL_dpix have been the same for one eager step: a loop that
    // changes the camera every iteration then runs eagerly instead of capturing graphs it never
    // replays
    const void* last_dpix = nullptr;
    int eager_since_change = 0;
    torch::Tensor guard;  // (1,) int32: ranks that overflowed in the last step (device, agreed)
    explicit Pool(torch::Device d)
        : dev(d),
          main(c10::hip::getStreamFromPoolMasqueradingAsCUDA(false, d.index())),
          side(c10::hip::getStreamFromPoolMasqueradingAsCUDA(false, d.index())) {}
    static void* geom_cb(void* c, size_t n) { return Arena::cb(&static_cast<Pool*>(c)->geom, n); }
    static void* bin_cb(void* c, size_t n) { return Arena::cb(&static_cast<Pool*>(c)->bin, n); }
    static void* img_cb(void* c, size_t n) { return Arena::cb(&static_cast<Pool*>(c)->img, n); }
};

static constexpr int kStatusWords = 16;  // per rank: nb header counts, band K (nb <= 15)
// then 3 x grid_y words of row statistics (GSR_FLAG_ROW_SPANS): the footer is foot_words_ long

ShardStep::ShardStep(Exchange& ex, const RasterCamera& cam, const ShardInputs& in, std::array<float, 3> bg,
                     double headroom, bool graph, int lag)
    : ex_(ex), cam_(cam), ccam_(cam.to_c()), in_(in.inputs()), headroom_(headroom),
      graph_(graph && ex.capturable()), lag_(std::max(lag, 1)), world_(ex.world()), rank_(ex.rank()) {
    TORCH_CHECK(in.means3D.defined() && in.means3D.is_cuda(), "ShardStep: means3D must be a device tensor");
    TORCH_CHECK(world_ >= 1 && world_ < kStatusWords, "ShardStep: 1..15 ranks");
    rs_.bg = bg;
    rs_.sh_degree = in.sh_degree;
    rs_.scale_modifier = in.scale_modifier;
    P_ = in.means3D.size(0);
    std::tie(g0_, g1_) = gaussian_shard(P_, world_, rank_);
    grid_y_ = (cam.height + GSR_TILE - 1) / GSR_TILE;
    TORCH_CHECK(world_ <= grid_y_, "ShardStep: more ranks than tile rows");
    rows_ = equal_bands(grid_y_, world_);
    foot_words_ = kStatusWords + 3 * grid_y_;
    pool_ = std::make_unique<Pool>(in.means3D.device());
    for (int i = 0; i < lag_ + 2; ++i) {
        pool_->ring.push_back(torch::empty({(int64_t)world_, (int64_t)foot_words_},
                                           torch::TensorOptions().dtype(torch::kInt32).pinned_memory(true)));
        pool_->ring_ev.push_back(std::make_unique<c10::Event>(c10::DeviceType::CUDA));
    }
}

ShardStep::~ShardStep() = default;

bool ShardStep::graph_active() const { return pool_ && pool_->graph != nullptr; }

void ShardStep::drop_graph() {
    pool_->graph.reset();
    pool_->graph_dpix = nullptr;
    pool_->eager_since_change = 0;
}

torch::Tensor ShardStep::overflow_guard() const { return pool_->guard; }

gsr_raster_settings ShardStep::band_settings() const {
    RasterSettings rs = rs_;
    rs.tile_y0 = rows_[rank_];
    rs.tile_y1 = rows_[rank_ + 1];
    rs.max_rendered = capacity_;
    return detail::make_settings(rs);
}

void ShardStep::size_buffers() {
    Pool& p = *pool_;
    drop_graph();
    const int nb = world_;
    const auto u8 = torch::TensorOptions().dtype(torch::kUInt8).device(p.dev);
    const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(p.dev);
    const int64_t Ps = g1_ - g0_;
    p.block_bytes = gsr_exchange_block_bytes(pair_cap_);
    p.grad_block = (size_t)pair_cap_ * GSR_SPLAT_GRAD_BYTES;
    p.send = torch::empty({(int64_t)(nb * p.block_bytes)}, u8);
    p.recv = torch::empty({(int64_t)(nb * p.block_bytes)}, u8);
    p.state = torch::empty({(int64_t)gsr_shard_state_bytes((int32_t)Ps, nb, pair_cap_)}, u8);
    p.radii = torch::empty({Ps}, f32.dtype(torch::kInt32));
    p.color = torch::zeros({3, cam_.height, cam_.width}, f32);
    p.g2 = torch::empty({(int64_t)nb * pair_cap_, GSR_GRAD2D_STRIDE}, f32);
    p.back = torch::empty({(int64_t)(nb * p.grad_block)}, u8);
    int tall = 1;
    for (int r = 0; r < world_; ++r) {
        const int a = std::min(rows_[r] * GSR_TILE, cam_.height), b = std::min(rows_[r + 1] * GSR_TILE, cam_.height);
        tall = std::max(tall, b - a);
    }
    p.tall = tall;
    p.status_off = (size_t)3 * tall * cam_.width;
    p.mine_floats = p.status_off + foot_words_;
    p.mine = torch::zeros({(int64_t)p.mine_floats}, f32);
    p.gathered = torch::empty({(int64_t)world_, (int64_t)p.mine_floats}, f32);
    p.image = torch::empty({3, cam_.height, cam_.width}, f32);
    p.guard = torch::zeros({1}, f32.dtype(torch::kInt32));
    p.lg = detail::LeafGrads(in_, Ps, /*want_conic=*/true);
    const detail::LeafGrads& l = p.lg;
    p.grads = {{"means2D", l.means2D}, {"conic", l.conic}, {"opacities", l.opac}, {"means3D", l.means3D},
               {"colors", l.colors},   {"sh_dc", l.dc},    {"sh_rest", l.rest},   {"cov3D", l.cov},
               {"scales", l.scales},   {"rotations", l.rots}};
    for (auto it = p.grads.begin(); it != p.grads.end();) it = it->second.defined() ? std::next(it) : p.grads.erase(it);
    for (Arena* a : {&p.geom, &p.bin, &p.img, &p.scratch}) {
        a->slots.clear();
        a->frozen = false;
    }
}

void ShardStep::plan() {
    const Stream cs = current_stream();
    const hipStream_t s = cs.stream();
    const gsr_gaussians g = shard_gaussians();
    const gsr_raster_settings rs = detail::make_settings(rs_);
    auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(pool_->dev);
    const int nb = world_;
    rows_ = equal_bands(grid_y_, world_);
    std::vector<int32_t> rows32(rows_.begin(), rows_.end());
    // probe 1: the shard's per-tile-row instance histogram (pair_cap 0: headers only)
    auto hist = torch::zeros({grid_y_}, i32);
    auto send0 = torch::empty({(int64_t)(nb * gsr_exchange_block_bytes(0))}, i32.dtype(torch::kUInt8));
    auto state0 = torch::empty({(int64_t)gsr_shard_state_bytes(g.P, nb, 0)}, i32.dtype(torch::kUInt8));
    auto radii0 = torch::empty({(int64_t)std::max(g.P, 1)}, i32);
    detail::check(gsr_shard_forward(&ccam_, &g, &rs, nb, rows32.data(), 0, send0.data_ptr(), radii0.data_ptr<int32_t>(),
                                    state0.data_ptr(), reinterpret_cast<uint32_t*>(hist.data_ptr<int32_t>()), s),
                  "gsr_shard_forward (probe)");
    auto hist64 = hist.to(torch::kInt64).bitwise_and(0xFFFFFFFFLL).contiguous();  // u32 counts, widened
    ex_.all_reduce_i64(hist64.data_ptr<int64_t>(), (size_t)grid_y_, false, s);
    auto hc = hist64.cpu();
    std::vector<int64_t> counts(hc.data_ptr<int64_t>(), hc.data_ptr<int64_t>() + grid_y_);
    rows_ = balance_bands(counts, world_);
    rows32.assign(rows_.begin(), rows_.end());
    // probe 2: splats per (shard, band) with the balanced cuts
    detail::check(gsr_shard_forward(&ccam_, &g, &rs, nb, rows32.data(), 0, send0.data_ptr(), radii0.data_ptr<int32_t>(),
                                    state0.data_ptr(), nullptr, s),
                  "gsr_shard_forward (probe)");
    const int64_t bb0 = (int64_t)gsr_exchange_block_bytes(0);
    auto heads = send0.view(torch::kInt32).view({nb, bb0 / 4}).select(1, 0).to(torch::kInt64);
    heads = heads.bitwise_and(0xFFFFFFFFLL).max().reshape({1}).contiguous();
    ex_.all_reduce_i64(heads.data_ptr<int64_t>(), 1, true, s);
    const int64_t pc = heads.cpu().item<int64_t>();
    const int64_t pair_cap = capacity_with_headroom(pc, headroom_);
    band_k_.assign(world_, 0);
    for (int b = 0; b < world_; ++b)
        for (int y = rows_[b]; y < rows_[b + 1]; ++y) band_k_[b] += counts[y];
    const int64_t kmax = *std::max_element(band_k_.begin(), band_k_.end());
    const int64_t cap = capacity_with_headroom(kmax, headroom_);
    require_int32_capacities(pair_cap, cap, world_);
    pair_cap_ = (int)pair_cap;
    capacity_ = (int)cap;
    pending_.clear();
    size_buffers();
}

void ShardStep::set_pair_cap(int pair_cap) {
    pair_cap_ = pair_cap;
    size_buffers();
}

void ShardStep::set_camera(const RasterCamera& cam) {
    TORCH_CHECK(cam.width == cam_.width && cam.height == cam_.height,
                "ShardStep::set_camera: the image size must stay the plan's");
    cam_ = cam;
    ccam_ = cam.to_c();
    drop_graph();  // the captured launches hold the old camera's values
    for (Arena* a : {&pool_->geom, &pool_->bin, &pool_->img, &pool_->scratch}) a->frozen = false;
}

void ShardStep::set_rebalance_every(int m) {
    TORCH_CHECK(m >= 0, "ShardStep: rebalance_every must be >= 0");
    rebalance_every_ = m;
}

// One step's work on the current stream (= the Pool's main stream, set by step()).  Called
// eagerly, or once under stream capture to record the graph that later steps replay.
void ShardStep::run(const torch::Tensor& dpix) {
    Pool& p = *pool_;
    const hipStream_t s = p.main.stream();
    const int nb = world_;
    const gsr_gaussians g = shard_gaussians();
    const gsr_raster_settings rs = detail::make_settings(rs_), bs = band_settings();
    std::vector<int32_t> rows32(rows_.begin(), rows_.end());
    for (Arena* a : {&p.geom, &p.bin, &p.img, &p.scratch}) a->next = 0;
    // 1. F1 on the shard + splat packing; with live re-planning the shard's row statistics
    //    (instances per tile row, rect start / end rows) go straight into this rank's status
    //    footer (zeroed by the previous step's gsr_gather_finish, or by size_buffers)
    float* const stats = p.mine.data_ptr<float>() + p.status_off + kStatusWords;
    gsr_raster_settings rss = rs;
    if (live_) rss.flags |= GSR_FLAG_ROW_SPANS;
    detail::check(gsr_shard_forward(&ccam_, &g, &rss, nb, rows32.data(), pair_cap_, p.send.data_ptr(),
                                    g.P ? p.radii.data_ptr<int32_t>() : nullptr, p.state.data_ptr(),
                                    live_ ? reinterpret_cast<uint32_t*>(stats) : nullptr, s),
                  "gsr_shard_forward");
    // 2. splats -> bands
    ex_.all_to_all(p.send.data_ptr(), p.recv.data_ptr(), p.block_bytes, s);
    // 3. F2..F6 on this band
    detail::check(gsr_band_forward(&ccam_, &bs, nb, pair_cap_, p.recv.data_ptr(), p.color.data_ptr<float>(),
                                   Pool::geom_cb, Pool::bin_cb, Pool::img_cb, &p, &p.bufs, s),
                  "gsr_band_forward");
    // 4. the band's pixels + status footer (send-header counts, band K) -> all-gather on the side
    //    stream, overlapping B1 (one launch: gsr_band_publish)
    detail::check(gsr_band_publish(&ccam_, &bs, p.tall, p.color.data_ptr<float>(), nb, p.send.data_ptr(), pair_cap_,
                                   &p.bufs, p.mine.data_ptr<float>(), (int64_t)p.status_off, s),
                  "gsr_band_publish");
    const bool overlap = ex_.capturable();
    if (overlap) {
        p.fork.record(p.main.unwrap());
        p.fork.block(p.side.unwrap());
    }
    ex_.all_gather(p.mine.data_ptr<float>(), p.gathered.data_ptr<float>(), p.mine_floats * sizeof(float),
                   overlap ? p.side.stream() : s);
    if (overlap) p.join.record(p.side.unwrap());
    // 5. B1 on the band, per-splat 2D gradients in the received slot layout
    detail::check(gsr_band_backward(&ccam_, &bs, nb, pair_cap_, &p.bufs, dpix.data_ptr<float>(), Arena::cb,
                                    &p.scratch, p.g2.data_ptr<float>(), s),
                  "gsr_band_backward");
    // 6. gradients -> owning shards
    ex_.all_to_all(p.g2.data_ptr<float>(), p.back.data_ptr(), p.grad_block, s);
    // 7. band-order sums + B2 on the shard
    detail::check(gsr_shard_backward(&ccam_, &g, &rs, nb, rows32.data(), pair_cap_, p.state.data_ptr(),
                                     p.back.data_ptr(), &p.lg.gg, s),
                  "gsr_shard_backward");
    // 8. join the all-gather; one launch (gsr_gather_finish) unpacks the bands into the full image,
    //    writes the agreed overflow word (the number of ranks whose splat counts or band K exceeded
    //    the plan's capacities in THIS step, the same on every rank; the optimizer guard of a
    //    training loop, no host wait) and clears this rank's row statistics for the next step
    if (overlap) p.join.block(p.main.unwrap());
    detail::check(gsr_gather_finish(&ccam_, world_, rows32.data(), p.tall, p.gathered.data_ptr<float>(),
                                    (int64_t)p.mine_floats, (int64_t)p.status_off, pair_cap_, capacity_,
                                    p.image.data_ptr<float>(), p.guard.data_ptr<int32_t>(), stats,
                                    live_ ? 3 * (int64_t)grid_y_ : 0, s),
                  "gsr_gather_finish");
}

void ShardStep::set_graph(bool on) {
    const bool g = on && ex_.capturable();
    if (g == graph_) return;
    graph_ = g;
    drop_graph();
}

void ShardStep::set_live_replan(bool on) {
    if (on == live_) return;
    live_ = on;
    drop_graph();  // the captured pack collects the statistics or not
}

void ShardStep::push_status() {
    Pool& p = *pool_;
    // poll(false) at the start of every step leaves at most lag_ older entries pending
    TORCH_CHECK(pending_.size() < p.ring.size(), "ShardStep: overflow ring full");
    const int slot = ring_next_;
    ring_next_ = (ring_next_ + 1) % (int)p.ring.size();
    // (a hipMemcpy2DAsync straight into the pinned slot would skip the gather into a contiguous
    // temporary, but it makes this object reference the HIP runtime directly, which the C++
    // executables must not link a second copy of: _build._exe_flags)
    auto st = p.gathered.narrow(1, (int64_t)p.status_off, foot_words_).contiguous().view(torch::kInt32);
    p.ring[slot].copy_(st, /*non_blocking=*/true);
    p.ring_ev[slot]->record(p.main.unwrap());
    pending_.push_back({steps_, slot, pair_cap_, capacity_, live_});
}

void ShardStep::poll(bool wait_all) {
    // the step exactly lag_ back (and anything older) is checked on every rank at the same call
    while (!pending_.empty() && (wait_all || pending_.front().step <= steps_ - lag_)) {
        const Pending q = pending_.front();
        pool_->ring_ev[q.slot]->synchronize();
        pending_.erase(pending_.begin());
        const int32_t* st = pool_->ring[q.slot].data_ptr<int32_t>();
        for (int r = 0; r < world_; ++r) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(st + r * foot_words_);
            std::vector<int64_t> counts(w, w + world_);
            const int64_t k = w[world_];
            if (*std::max_element(counts.begin(), counts.end()) > q.pair_cap || k > q.capacity) {
                pending_.clear();
                throw ShardOverflowError(q.step, r, counts, q.pair_cap, k, q.capacity);
            }
        }
        if (q.stats) {  // a step without statistics (live re-planning off) leaves the last ones
            last_stats_.assign(st, st + (size_t)world_ * foot_words_);
            last_stats_step_ = q.step;
        }
    }
}

void ShardStep::replan_live() {
    if (last_stats_step_ < 0 || last_stats_step_ == stats_used_step_) return;
    stats_used_step_ = last_stats_step_;
    const int gy = grid_y_;
    std::vector<int64_t> inst(gy, 0);
    std::vector<std::vector<int64_t>> starts(world_, std::vector<int64_t>(gy)), ends = starts;
    for (int r = 0; r < world_; ++r) {
        const uint32_t* f = reinterpret_cast<const uint32_t*>(last_stats_.data() + (size_t)r * foot_words_) + kStatusWords;
        for (int y = 0; y < gy; ++y) {
            inst[y] += f[y];
            starts[r][y] = f[gy + y];
            ends[r][y] = f[2 * gy + y];
        }
    }
    const StatsPlan sp = plan_from_stats(inst, starts, ends, world_);
    const int64_t kmax = *std::max_element(sp.band_k.begin(), sp.band_k.end());
    const int64_t pc_need = std::max<int64_t>(sp.max_splats, 1), cap_need = std::max<int64_t>(kmax, 1);
    const int64_t pc = capacity_with_headroom(pc_need, headroom_), cap = capacity_with_headroom(cap_need, headroom_);
    const bool short_caps = pc_need > pair_cap_ || cap_need > capacity_;
    const bool fat_caps = pair_cap_ > 2 * pc || capacity_ > 2 * cap;
    if (sp.rows == rows_ && !short_caps && !fat_caps) return;
    require_int32_capacities(pc, cap, world_);
    rows_ = sp.rows;
    band_k_ = sp.band_k;
    pair_cap_ = (int)pc;
    capacity_ = (int)cap;
    size_buffers();  // new cuts / capacities: buffers re-sized, the captured graph dropped
    ++live_replans_;
}

void ShardStep::check() { poll(true); }

int64_t ShardStep::band_num_rendered() const {
    void* k = const_cast<void*>(gsr_view(&ccam_, world_ * pair_cap_, &pool_->bufs, GSR_VIEW_COUNTS));
    TORCH_CHECK(k != nullptr && steps_ > 0, "ShardStep: no step yet");
    return (int64_t)(uint32_t)dev_view(k, 1, torch::kInt32).item<int32_t>();
}

ShardStep::Result ShardStep::step(const torch::Tensor& dL_dpix) {
    TORCH_CHECK(pair_cap_ > 0 && capacity_ > 0, "ShardStep: call plan() first");
    TORCH_CHECK(dL_dpix.is_cuda() && dL_dpix.scalar_type() == torch::kFloat32 && dL_dpix.is_contiguous() &&
                    dL_dpix.numel() == (int64_t)3 * cam_.height * cam_.width,
                "ShardStep: dL_dpix must be a contiguous (3,H,W) f32 device tensor");
    if (rebalance_every_ > 0 && steps_ > 0 && steps_ % rebalance_every_ == 0) {
        poll(true);  // the old plan's pending checks first
        plan();      // drops the graph; this step runs eagerly and captures again
        ++replans_;
    }
    poll(false);
    if (live_) replan_live();
    Pool& p = *pool_;
    // the step runs on its own stream (capturable), ordered after / before the caller's
    const Stream caller = current_stream();
    p.enter.record(caller.unwrap());
    p.enter.block(p.main.unwrap());
    {
        StreamGuard guard(p.main.unwrap());
        if (graph_ && p.graph && p.graph_dpix == dL_dpix.data_ptr()) {
            p.graph->replay();
        } else {
            run(dL_dpix);  // this step's result, eagerly
            const bool stable = p.eager_since_change > 0 && p.last_dpix == dL_dpix.data_ptr();
            p.last_dpix = dL_dpix.data_ptr();
            ++p.eager_since_change;
            if (graph_ && stable) {
                // every arena slot now exists: capture the same calls on the same buffers
                drop_graph();
                for (Arena* a : {&p.geom, &p.bin, &p.img, &p.scratch}) a->frozen = true;
                p.main.unwrap().synchronize();
                p.graph = std::make_unique<at::cuda::CUDAGraph>();
                p.graph->capture_begin({0, 0}, hipStreamCaptureModeRelaxed);
                try {
                    run(dL_dpix);
                } catch (...) {
                    try {
                        p.graph->capture_end();
                    } catch (...) {
                    }
                    drop_graph();
                    throw;
                }
                p.graph->capture_end();
                p.graph_dpix = dL_dpix.data_ptr();
            }
        }
        push_status();
    }
    p.leave.record(p.main.unwrap());
    p.leave.block(caller.unwrap());
    ++steps_;
    return {p.image, p.grads, p.radii};
}

}  // namespace gsr
