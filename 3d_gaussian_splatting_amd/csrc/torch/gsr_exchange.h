// gsr_exchange.h -- the transports of the multi-GPU step.  The collectives of
// gsr::ShardStep go through an `Exchange`: RCCL over xGMI (grouped ncclSend / ncclRecv for the
// all-to-alls, ncclAllGather for the bands) on the GPU box, a host-staged exchange through a
// c10d::Store for ranks that share one GPU (the two-process test; RCCL refuses two ranks on one
// device), or an in-process rank group for the one-GPU rehearsal.
#pragma once
#include <hip/hip_runtime.h>  // hipStream_t only: the transports use libtorch streams and events
#include <torch/torch.h>

#include <c10/core/Event.h>

#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

namespace c10d {
class Store;
}

namespace gsr {

class Exchange {
   public:
    virtual ~Exchange() = default;
    virtual int rank() const = 0;
    virtual int world() const = 0;
    virtual bool capturable() const = 0;  // may be recorded into a hipGraph
    virtual const char* name() const = 0;
    // the transport's own count of ranks (RCCL: ncclCommCount), for reports
    virtual int comm_world() const { return world(); }
    // block b of `send` (block_bytes each) -> rank b; block s of `recv` <- rank s
    virtual void all_to_all(const void* send, void* recv, size_t block_bytes, hipStream_t s) = 0;
    // `bytes` from every rank into recv, rank-major
    virtual void all_gather(const void* send, void* recv, size_t bytes, hipStream_t s) = 0;
    // in place over ranks (setup only)
    virtual void all_reduce_i64(int64_t* buf, size_t n, bool max, hipStream_t s) = 0;
};

// RCCL: rank 0 makes the unique id, the caller broadcasts it (torch.distributed, a store, ...).
std::vector<uint8_t> rccl_unique_id();
std::unique_ptr<Exchange> rccl_exchange(const std::vector<uint8_t>& unique_id, int rank, int world);
// RCCL with the id passed through a c10d::Store (key "gsr/rccl_id").
std::unique_ptr<Exchange> rccl_exchange(c10d::Store& store, int rank, int world);
// Host-staged through a c10d::Store (device -> host -> store -> host -> device); not capturable.
std::unique_ptr<Exchange> store_exchange(std::shared_ptr<c10d::Store> store, int rank, int world);

// In-process rank group (one-GPU rehearsal of the N-rank step, scripts/band_sim.py --cpp): every
// rank's ShardStep runs in its own host thread on the same device, and the collectives are
// device-to-device copies between the ranks' own buffers, ordered by events and host barriers.
// After a live step each exchange keeps what it delivered (recv blocks, gathered rows, gradient
// blocks); in replay mode it copies those instead of waiting for peers, so ONE rank's whole C++
// step (glue, graph replay and exchange-sized copies included) can be timed alone on the GPU.
class LocalGroup {
   public:
    explicit LocalGroup(int world) : world_(world), pub_(world), fin_(world), host_(world) {}
    int world() const { return world_; }
    void barrier() {
        std::unique_lock<std::mutex> lk(mu_);
        const int64_t gen = gen_;
        if (++count_ == world_) {
            count_ = 0;
            ++gen_;
            cv_.notify_all();
        } else {
            cv_.wait(lk, [&] { return gen_ != gen; });
        }
    }
    struct Pub {
        const void* ptr = nullptr;
        c10::Event* ev = nullptr;
    };
    std::vector<Pub> pub_;             // per rank: its send buffer and the event after it was written
    std::vector<c10::Event*> fin_;     // per rank: the event after its copies from the peers
    std::vector<std::vector<int64_t>> host_;  // all-reduce contributions

   private:
    int world_;
    std::mutex mu_;
    std::condition_variable cv_;
    int count_ = 0;
    int64_t gen_ = 0;
};
std::shared_ptr<LocalGroup> local_group(int world);
std::unique_ptr<Exchange> local_exchange(std::shared_ptr<LocalGroup> group, int rank);
// replay: copy the last live step's deliveries (copies) or move nothing (the receive buffers
// still hold them); throws unless ex is a local exchange
void local_exchange_set_replay(Exchange& ex, bool on, bool copies = true);

namespace detail {
// a device tensor over raw device memory (no ownership)
torch::Tensor dev_view(void* p, int64_t n, torch::ScalarType t);
}  // namespace detail

}  // namespace gsr
