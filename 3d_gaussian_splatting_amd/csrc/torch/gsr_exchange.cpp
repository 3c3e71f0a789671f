// gsr_exchange.cpp -- the transports of the multi-GPU step (see gsr_exchange.h):
// RCCL through the C ABI of libgsr_hip.so, a host-staged exchange through a c10d::Store, and the
// in-process rank group of the one-GPU rehearsal.
#include "gsr_exchange.h"

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/StreamGuard.h>
#include <torch/csrc/distributed/c10d/Store.hpp>

#include "gsr/gsr_comm.h"
#include "gsr_render.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

namespace gsr {
namespace detail {
torch::Tensor dev_view(void* p, int64_t n, torch::ScalarType t) {
    return torch::from_blob(p, {n}, torch::TensorOptions().dtype(t).device(torch::kCUDA, c10::hip::current_device()));
}
}  // namespace detail

namespace {

constexpr int kMaxLocalRanks = 16;

using Stream = c10::hip::HIPStreamMasqueradingAsCUDA;
// c10's device-generic guard and events (they dispatch through the registered HIP guard
// implementation): this file then references no HIP runtime symbol itself, so an executable
// linking it keeps libtorch's one HIP runtime (tests/test_native_abi.py).
using StreamGuard = c10::StreamGuard;
using detail::dev_view;

Stream current_stream() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(); }

// ---- RCCL exchange: the C ABI of libgsr_hip.so (include/gsr/gsr_comm.h) ----
class RcclExchange final : public Exchange {
   public:
    RcclExchange(const std::vector<uint8_t>& id, int rank, int world) : rank_(rank), world_(world) {
        if (id.size() != GSR_COMM_ID_BYTES) throw std::invalid_argument("rccl: bad unique id size");
        detail::check(gsr_comm_init(&comm_, id.data(), world, rank), "gsr_comm_init");
    }
    ~RcclExchange() override { (void)gsr_comm_destroy(comm_); }
    int rank() const override { return rank_; }
    int world() const override { return world_; }
    bool capturable() const override { return true; }
    const char* name() const override { return "rccl"; }
    int comm_world() const override {
        int32_t n = 0, r = 0;
        detail::check(gsr_comm_size(comm_, &n, &r), "gsr_comm_size");
        return n;
    }
    void all_to_all(const void* send, void* recv, size_t bb, hipStream_t s) override {
        detail::check(gsr_comm_all_to_all(comm_, send, recv, bb, s), "gsr_comm_all_to_all");
    }
    void all_gather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
        detail::check(gsr_comm_all_gather(comm_, send, recv, bytes, s), "gsr_comm_all_gather");
    }
    void all_reduce_i64(int64_t* buf, size_t n, bool max, hipStream_t s) override {
        detail::check(gsr_comm_all_reduce_i64(comm_, buf, n, max ? 1 : 0, s), "gsr_comm_all_reduce_i64");
    }

   private:
    int rank_, world_;
    gsr_comm* comm_ = nullptr;
};

// ---- host-staged exchange through a c10d::Store (ranks sharing one GPU) ----
class StoreExchange final : public Exchange {
   public:
    // Every rank announces itself under this exchange's join key (exchanges are created in the
    // same order on every rank, so the per-process counter names the same key everywhere) and
    // waits until `world` ranks have: comm_world() is then the store's own count of the ranks
    // that joined, not the number the caller claimed.
    StoreExchange(std::shared_ptr<c10d::Store> store, int rank, int world)
        : store_(std::move(store)), rank_(rank), world_(world) {
        static int instances = 0;
        join_key_ = "gsr/join/" + std::to_string(instances++);
        store_->add(join_key_, 1);
        for (int spin = 0; store_->add(join_key_, 0) < world_; ++spin) {
            if (spin > 600000) throw std::runtime_error("store exchange: ranks did not join within 120 s");
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    }
    int rank() const override { return rank_; }
    int world() const override { return world_; }
    bool capturable() const override { return false; }
    const char* name() const override { return "store"; }
    int comm_world() const override { return (int)store_->add(join_key_, 0); }
    void all_to_all(const void* send, void* recv, size_t bb, hipStream_t s) override {
        const std::string tag = "gsr/a2a/" + std::to_string(seq_++) + "/";
        std::vector<uint8_t> h((size_t)world_ * bb);
        d2h(h.data(), send, h.size(), s);
        for (int p = 0; p < world_; ++p)
            put(tag + std::to_string(rank_) + ">" + std::to_string(p), h.data() + (size_t)p * bb, bb);
        for (int p = 0; p < world_; ++p) {
            const std::string key = tag + std::to_string(p) + ">" + std::to_string(rank_);
            take(key, h.data() + (size_t)p * bb, bb, /*erase=*/true);
        }
        h2d(recv, h.data(), h.size(), s);
    }
    void all_gather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
        const std::string tag = "gsr/ag/" + std::to_string(seq_++) + "/";
        std::vector<uint8_t> h(bytes);
        d2h(h.data(), send, bytes, s);
        put(tag + std::to_string(rank_), h.data(), bytes);
        std::vector<uint8_t> all((size_t)world_ * bytes);
        for (int p = 0; p < world_; ++p) take(tag + std::to_string(p), all.data() + (size_t)p * bytes, bytes, false);
        barrier(tag);
        release(tag, bytes);
        h2d(recv, all.data(), all.size(), s);
    }
    void all_reduce_i64(int64_t* buf, size_t n, bool max, hipStream_t s) override {
        std::vector<int64_t> mine(n), acc(n);
        all_gather_host(mine, buf, n, s, acc, max);
        h2d(buf, acc.data(), n * sizeof(int64_t), s);
    }

   private:
    void all_gather_host(std::vector<int64_t>& mine, const int64_t* dev, size_t n, hipStream_t s,
                         std::vector<int64_t>& acc, bool max) {
        d2h(mine.data(), dev, n * sizeof(int64_t), s);
        const std::string tag = "gsr/ar/" + std::to_string(seq_++) + "/";
        std::vector<uint8_t> b(n * sizeof(int64_t));
        std::memcpy(b.data(), mine.data(), b.size());
        store_->set(tag + std::to_string(rank_), b);
        for (int p = 0; p < world_; ++p) {
            auto v = store_->get(tag + std::to_string(p));
            const int64_t* x = reinterpret_cast<const int64_t*>(v.data());
            for (size_t i = 0; i < n; ++i) acc[i] = p == 0 ? x[i] : (max ? std::max(acc[i], x[i]) : acc[i] + x[i]);
        }
        barrier(tag);
        release(tag);
    }
    void barrier(const std::string& tag) {
        store_->add(tag + "done", 1);
        while (store_->add(tag + "done", 0) < world_) std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    // After barrier(tag): every rank has read every payload, so the last rank to leave deletes the
    // payloads and both counters -- a long run leaves no keys behind in the store.
    void release(const std::string& tag, size_t bytes = 0) {
        if (store_->add(tag + "left", 1) < world_) return;
        for (int p = 0; p < world_; ++p) {
            if (bytes == 0) {
                store_->deleteKey(tag + std::to_string(p));
            } else {
                for (size_t c = 0; c < chunks(bytes); ++c) store_->deleteKey(tag + std::to_string(p) + "#" + std::to_string(c));
            }
        }
        store_->deleteKey(tag + "done");
        store_->deleteKey(tag + "left");
    }
    // Values go through the store in pieces of at most kChunk bytes (the libuv TCPStore refuses
    // payloads above 8 MiB; a 1M / 1080p splat block for 2 ranks is 17.8 MB).  The reader knows the
    // size, hence the number of pieces.
    static constexpr size_t kChunk = 4u << 20;
    static size_t chunks(size_t n) { return n == 0 ? 1 : (n + kChunk - 1) / kChunk; }
    void put(const std::string& key, const uint8_t* data, size_t n) {
        for (size_t c = 0; c < chunks(n); ++c) {
            const size_t a = c * kChunk, b = std::min(n, a + kChunk);
            store_->set(key + "#" + std::to_string(c), std::vector<uint8_t>(data + a, data + b));
        }
    }
    void take(const std::string& key, uint8_t* out, size_t n, bool erase) {
        for (size_t c = 0; c < chunks(n); ++c) {
            const std::string k = key + "#" + std::to_string(c);
            auto v = store_->get(k);
            const size_t a = c * kChunk, want = std::min(n, a + kChunk) - a;
            if (v.size() != want) throw std::runtime_error("store exchange: block size mismatch");
            std::memcpy(out + a, v.data(), want);
            if (erase) store_->deleteKey(k);
        }
    }
    // synchronous copies on the caller's current stream (the step runs with it set to its own)
    static void d2h(void* h, const void* d, size_t n, hipStream_t) {
        auto src = dev_view(const_cast<void*>(d), (int64_t)n, torch::kUInt8);
        torch::from_blob(h, {(int64_t)n}, torch::kUInt8).copy_(src);
    }
    static void h2d(void* d, const void* h, size_t n, hipStream_t) {
        dev_view(d, (int64_t)n, torch::kUInt8).copy_(torch::from_blob(const_cast<void*>(h), {(int64_t)n}, torch::kUInt8));
        current_stream().unwrap().synchronize();  // h is a host buffer of this call
    }
    std::shared_ptr<c10d::Store> store_;
    int rank_, world_;
    int64_t seq_ = 0;
    std::string join_key_;
};

// ---- in-process rank group (one-GPU rehearsal; LocalGroup itself: gsr_exchange.h) ----
class LocalExchange final : public Exchange {
   public:
    LocalExchange(std::shared_ptr<LocalGroup> g, int rank) : g_(std::move(g)), rank_(rank) {
        if (rank < 0 || rank >= g_->world()) throw std::invalid_argument("local exchange: rank out of range");
    }
    int rank() const override { return rank_; }
    int world() const override { return g_->world(); }
    bool capturable() const override { return replay_; }
    const char* name() const override { return replay_ ? "local-replay" : "local"; }
    // copies = false: replay without moving any bytes -- the step's receive buffers still hold
    // the last delivery, so the results are the same and the time is the rank's compute + glue
    void set_replay(bool on, bool copies) {
        if (on && snap_.size() < 3) throw std::runtime_error("local exchange: replay needs one live step first");
        replay_ = on;
        replay_copies_ = copies;
    }
    void all_to_all(const void* send, void* recv, size_t bb, hipStream_t s) override {
        const int w = g_->world();
        deliver(s, send, recv, (size_t)w * bb, /*always=*/false, [&](int p, const char* src) {
            copy(static_cast<char*>(recv) + (size_t)p * bb, src + (size_t)rank_ * bb, bb);
        });
    }
    // (the image all-gather runs on the step's side stream, overlapping B1: replayed with its
    // copy in both replay modes, as RCCL's would overlap -- and so that the side stream's branch
    // of a captured graph is never empty)
    void all_gather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
        deliver(s, send, recv, (size_t)g_->world() * bytes, /*always=*/true, [&](int p, const char* src) {
            copy(static_cast<char*>(recv) + (size_t)p * bytes, src, bytes);
        });
    }
    void all_reduce_i64(int64_t* buf, size_t n, bool max, hipStream_t) override {
        auto d = dev_view(buf, (int64_t)(n * sizeof(int64_t)), torch::kUInt8);
        std::vector<int64_t> mine(n);
        torch::from_blob(mine.data(), {(int64_t)(n * sizeof(int64_t))}, torch::kUInt8).copy_(d);
        g_->host_[rank_] = mine;
        g_->barrier();
        std::vector<int64_t> acc = g_->host_[0];
        for (int p = 1; p < g_->world(); ++p)
            for (size_t i = 0; i < n; ++i) acc[i] = max ? std::max(acc[i], g_->host_[p][i]) : acc[i] + g_->host_[p][i];
        g_->barrier();  // everyone has read every contribution
        d.copy_(torch::from_blob(acc.data(), {(int64_t)(n * sizeof(int64_t))}, torch::kUInt8));
        current_stream().unwrap().synchronize();  // acc is a host buffer of this call
    }

   private:
    static void copy(void* dst, const void* src, size_t n) {
        dev_view(dst, (int64_t)n, torch::kUInt8).copy_(dev_view(const_cast<void*>(src), (int64_t)n, torch::kUInt8));
    }
    // A step makes three calls in a fixed order (splats all-to-all, image all-gather, gradient
    // all-to-all): call k % 3 keeps its delivery for replay.  Every copy and event is on the
    // stream the step passed (its main stream, or the side stream of the overlapped all-gather).
    template <class F>
    void deliver(hipStream_t s, const void* send, void* recv, size_t total, bool always, F&& from_peer) {
        const int k = (int)(calls_++ % 3);
        const Stream cs = s ? c10::hip::getStreamFromExternalMasqueradingAsCUDA(s, c10::hip::current_device())
                            : current_stream();
        StreamGuard on(cs.unwrap());
        if (replay_) {
            if (replay_copies_ || always) copy(recv, snap_[k].data_ptr(), total);
            return;
        }
        ready_.record(cs.unwrap());
        g_->pub_[rank_] = {send, &ready_};
        g_->barrier();  // every rank's send buffer is published
        for (int p = 0; p < g_->world(); ++p) {
            g_->pub_[p].ev->block(cs.unwrap());
            from_peer(p, static_cast<const char*>(g_->pub_[p].ptr));
        }
        done_.record(cs.unwrap());
        g_->fin_[rank_] = &done_;
        g_->barrier();  // every rank has issued its copies (pub_ may be reused after the next barrier)
        for (int p = 0; p < g_->world(); ++p) g_->fin_[p]->block(cs.unwrap());  // peers done reading my send
        g_->barrier();  // fin_ read by everyone
        if ((int)snap_.size() <= k) snap_.resize(k + 1);
        if (!snap_[k].defined() || (size_t)snap_[k].numel() != total)
            snap_[k] = torch::empty({(int64_t)total}, torch::TensorOptions().dtype(torch::kUInt8).device(
                                                           torch::kCUDA, c10::hip::current_device()));
        copy(snap_[k].data_ptr(), recv, total);
    }
    std::shared_ptr<LocalGroup> g_;
    int rank_;
    bool replay_ = false, replay_copies_ = true;
    int64_t calls_ = 0;
    c10::Event ready_{c10::DeviceType::CUDA}, done_{c10::DeviceType::CUDA};
    std::vector<torch::Tensor> snap_;
};

}  // namespace

std::vector<uint8_t> rccl_unique_id() {
    std::vector<uint8_t> out(GSR_COMM_ID_BYTES);
    detail::check(gsr_comm_unique_id(out.data()), "gsr_comm_unique_id");
    return out;
}

std::unique_ptr<Exchange> rccl_exchange(const std::vector<uint8_t>& unique_id, int rank, int world) {
    return std::make_unique<RcclExchange>(unique_id, rank, world);
}

std::unique_ptr<Exchange> rccl_exchange(c10d::Store& store, int rank, int world) {
    std::vector<uint8_t> id;
    if (rank == 0) {
        id = rccl_unique_id();
        store.set("gsr/rccl_id", id);
    } else {
        id = store.get("gsr/rccl_id");
    }
    return rccl_exchange(id, rank, world);
}

std::unique_ptr<Exchange> store_exchange(std::shared_ptr<c10d::Store> store, int rank, int world) {
    return std::make_unique<StoreExchange>(std::move(store), rank, world);
}

std::shared_ptr<LocalGroup> local_group(int world) {
    if (world < 1 || world > kMaxLocalRanks) throw std::invalid_argument("local group: 1..16 ranks");
    return std::make_shared<LocalGroup>(world);
}
std::unique_ptr<Exchange> local_exchange(std::shared_ptr<LocalGroup> group, int rank) {
    return std::make_unique<LocalExchange>(std::move(group), rank);
}
void local_exchange_set_replay(Exchange& ex, bool on, bool copies) {
    auto* l = dynamic_cast<LocalExchange*>(&ex);
    if (!l) throw std::invalid_argument("not a local exchange");
    l->set_replay(on, copies);
}

}  // namespace gsr
