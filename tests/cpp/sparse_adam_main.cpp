// sparse_adam_main.cpp -- the visibility-masked gsr::fused_adam_step(optimizers, radii) on libtorch's
// own Adam state, checked against the dense gsr::fused_adam_step (tests/test_gpu_sparse_adam.py).
//
// Six torch::optim::Adam instances (one parameter each, rows of 3 / 3 / 45 / 1 / 3 / 4 floats, the
// reference's learning rates) on seeded tensors.  Two sparse steps with two different masks; before
// each, parameters and Adam state are cloned into a second set of optimizers that takes the dense
// step with the same gradients (zero on the invisible rows, which hold NaN on the sparse side).
// Expected = where(row visible, dense, before), bit for bit, for the parameter and both moments.
// Every AdamParamState::step must advance by one per call; a radii tensor of the wrong dtype or of
// a length that does not divide the parameters must throw.  Exit status 0 only if all of it held.
#include <torch/torch.h>

#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "gsr_trainer.h"

namespace {
constexpr int64_t kP = 1027;
const int64_t kWidths[6] = {3, 3, 45, 1, 3, 4};
const double kLrs[6] = {0.00016, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001};
int g_failed = 0;

void expect(bool ok, const char* what, int step, int group) {
    if (ok) return;
    ++g_failed;
    std::fprintf(stderr, "FAILED: %s (step %d, group %d)\n", what, step, group);
}

struct Set {
    std::vector<torch::Tensor> params;
    std::vector<std::unique_ptr<torch::optim::Adam>> opts;
    std::vector<torch::optim::Adam*> list() const {
        std::vector<torch::optim::Adam*> v;
        for (auto& o : opts) v.push_back(o.get());
        return v;
    }
    torch::optim::AdamParamState& state(int i) {
        return static_cast<torch::optim::AdamParamState&>(*opts[i]->state().at(params[i].unsafeGetTensorImpl()));
    }
};

Set make_set(const std::vector<torch::Tensor>& values) {
    Set s;
    for (int i = 0; i < 6; ++i) {
        auto p = values[i].clone().set_requires_grad(true);
        s.params.push_back(p);
        s.opts.push_back(std::make_unique<torch::optim::Adam>(std::vector<torch::Tensor>{p},
                                                              torch::optim::AdamOptions(kLrs[i])));
    }
    return s;
}

template <class F>
bool throws(F&& f) {
    try {
        f();
    } catch (const c10::Error&) {
        return true;
    }
    return false;
}
}  // namespace

int main() {
    if (!torch::cuda::is_available()) {
        std::fprintf(stderr, "no GPU\n");
        return 2;
    }
    torch::manual_seed(11);
    const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(torch::kCUDA);
    std::vector<torch::Tensor> init;
    for (int i = 0; i < 6; ++i) init.push_back(torch::randn({kP, kWidths[i]}, f32));
    Set sparse = make_set(init);

    // mask 0: random 40 %; mask 1: runs -- rows 100 .. 899 invisible, plus a negative radius
    std::vector<torch::Tensor> radii;
    radii.push_back((torch::rand({kP}, f32) < 0.4).to(torch::kInt32) * 7);
    auto runs = torch::full({kP}, 3, f32.dtype(torch::kInt32));
    runs.slice(0, 100, 900).zero_();
    runs[950] = -2;
    radii.push_back(runs);

    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int step = 0; step < 2; ++step) {
        const auto rows = (radii[step] > 0).unsqueeze(1);  // (P, 1), broadcasts over a row
        // the dense twin starts from the sparse side's parameters and state
        std::vector<torch::Tensor> before_p, before_m, before_v;
        for (int i = 0; i < 6; ++i) before_p.push_back(sparse.params[i].detach().clone());
        Set dense = make_set(before_p);
        std::vector<int64_t> steps_before(6, 0);
        for (int i = 0; i < 6; ++i) {
            auto g = torch::randn({kP, kWidths[i]}, f32);
            sparse.params[i].mutable_grad() = torch::where(rows, g, torch::full_like(g, nan));
            dense.params[i].mutable_grad() = torch::where(rows, g, torch::zeros_like(g));
            if (step > 0) {  // re-synchronise the twin's state from the sparse side
                auto& s = sparse.state(i);
                auto st = std::make_unique<torch::optim::AdamParamState>();
                st->step(s.step());
                st->exp_avg(s.exp_avg().clone());
                st->exp_avg_sq(s.exp_avg_sq().clone());
                dense.opts[i]->state()[dense.params[i].unsafeGetTensorImpl()] = std::move(st);
                steps_before[i] = s.step();
                before_m.push_back(s.exp_avg().clone());
                before_v.push_back(s.exp_avg_sq().clone());
            } else {
                before_m.push_back(torch::zeros_like(before_p[i]));
                before_v.push_back(torch::zeros_like(before_p[i]));
            }
        }
        const std::vector<torch::optim::Adam*> sl = sparse.list(), dl = dense.list();
        gsr::fused_adam_step(sl, radii[step]);
        gsr::fused_adam_step(dl);
        for (int i = 0; i < 6; ++i) {
            auto& s = sparse.state(i);
            auto& d = dense.state(i);
            expect(s.step() == steps_before[i] + 1, "AdamParamState::step advanced by one", step, i);
            expect(torch::equal(sparse.params[i].detach(), torch::where(rows, dense.params[i].detach(), before_p[i])),
                   "param == where(visible, dense, before)", step, i);
            expect(torch::equal(s.exp_avg(), torch::where(rows, d.exp_avg(), before_m[i])),
                   "exp_avg == where(visible, dense, before)", step, i);
            expect(torch::equal(s.exp_avg_sq(), torch::where(rows, d.exp_avg_sq(), before_v[i])),
                   "exp_avg_sq == where(visible, dense, before)", step, i);
            expect(!torch::equal(sparse.params[i].detach(), before_p[i]), "the visible rows moved", step, i);
        }
    }

    // refusals: before any state is touched
    const std::vector<torch::optim::Adam*> sl = sparse.list();
    const int64_t step0 = sparse.state(0).step();
    expect(throws([&] { gsr::fused_adam_step(sl, radii[0].to(torch::kInt64)); }), "int64 radii throws", 2, -1);
    expect(throws([&] { gsr::fused_adam_step(sl, radii[0].to(torch::kFloat32)); }), "float radii throws", 2, -1);
    expect(throws([&] { gsr::fused_adam_step(sl, radii[0].slice(0, 0, kP - 1).contiguous()); }),
           "radii of a length that does not divide the parameters throws", 2, -1);
    expect(throws([&] { gsr::fused_adam_step(sl, radii[0].cpu()); }), "host radii throws", 2, -1);
    expect(sparse.state(0).step() == step0, "a refused call leaves the step counts alone", 2, 0);

    torch::cuda::synchronize();
    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("sparse adam ok: 2 steps x 6 groups, P = %lld\n", (long long)kP);
    return 0;
}
