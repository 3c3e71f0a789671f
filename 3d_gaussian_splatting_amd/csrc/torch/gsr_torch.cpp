// gsr_torch.cpp -- libtorch layer over the C ABI: the tensor-to-ABI glue (gsr_render.h detail::),
// the RasterizeGaussians autograd Functions and the render() helpers.  Host C++ only: every byte
// of device work goes through include/gsr/gsr.h into libgsr_hip.so (no torch types cross that
// ABI).  The Python binding of this layer is gsr_bind.cpp.
//
// Scratch buffers (geometry / binning / image) are uint8 tensors from torch's caching
// allocator, created inside the C ABI's allocation callbacks and kept in the autograd context
// until backward -- the library itself allocates nothing persistent.
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/Event.h>
#include <c10/hip/HIPStream.h>
#include <torch/torch.h>

#include <cmath>
#include <cstdio>
#include <stdexcept>

#include "gsr_render.h"

namespace gsr {
namespace detail {
void check(int rc, const char* what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " +
                                          gsr_last_error());
}
void* current_stream() { return (void*)c10::hip::getCurrentHIPStream().stream(); }

// absent optional inputs travel through autograd as defined 0-element tensors (undefined
// tensors are rejected by Function::apply's input bookkeeping)
bool present(const torch::Tensor& t) { return t.defined() && t.numel() > 0; }

gsr_gaussians make_gaussians(const Inputs& in, int sh_degree, float scale_modifier, int64_t g0, int64_t g1) {
    gsr_gaussians g{};
    const int64_t P = in.means3D.size(0);
    if (g1 < 0) g1 = P;
    TORCH_CHECK(0 <= g0 && g0 <= g1 && g1 <= P, "rows [", g0, ", ", g1, ") outside the ", P, " Gaussians");
    auto rows = [&](const torch::Tensor& t, const char* name, int64_t per) -> const float* {
        if (!present(t)) return nullptr;
        TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
        TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32");
        TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
        TORCH_CHECK(t.numel() == P * per, name, " has ", t.numel(), " elements, expected ", P * per);
        return t.data_ptr<float>() + g0 * per;
    };
    g.P = (int32_t)(g1 - g0);
    g.sh_degree = sh_degree;
    g.scale_modifier = scale_modifier;
    g.means3D = rows(in.means3D, "means3D", 3);
    g.opacities = rows(in.opac, "opacities", 1);
    if (present(in.colors)) {
        g.colors_precomp = rows(in.colors, "colors_precomp", 3);
        g.sh_degree = 0;
    } else {
        g.sh_dc = rows(in.sh_dc, "sh_dc", 3);
        if (present(in.sh_rest)) {
            const int64_t M = in.sh_rest.numel() / std::max<int64_t>(P, 1) / 3;
            g.sh_rest = rows(in.sh_rest, "sh_rest", 3 * M);
            g.sh_rest_coeffs = (int32_t)M;
        }
    }
    if (present(in.cov3D)) {
        g.cov3D_precomp = rows(in.cov3D, "cov3D_precomp", 6);
    } else {
        g.scales = rows(in.scales, "scales", 3);
        g.rotations = rows(in.rots, "rotations", 4);
    }
    return g;
}

gsr_raster_settings make_settings(const RasterSettings& rs) {
    gsr_raster_settings s{};
    for (int c = 0; c < 3; ++c) s.bg[c] = rs.bg[c];
    s.tile_y0 = rs.tile_y0;
    s.tile_y1 = rs.tile_y1;
    s.flags = (rs.debug ? GSR_FLAG_DEBUG : 0u) | (rs.antialiasing ? GSR_FLAG_ANTIALIAS : 0u);
    s.max_rendered = rs.max_rendered;
    return s;
}

LeafGrads::LeafGrads(const Inputs& in, int64_t rows, bool want_conic) {
    const auto fo = in.means3D.options();
    auto out = [&](torch::Tensor& t, std::initializer_list<int64_t> shape) {
        t = torch::empty(shape, fo);
        return t.data_ptr<float>();
    };
    gg.dL_dmeans2D = out(means2D, {rows, 3});
    if (want_conic) gg.dL_dconic = out(conic, {rows, 3});
    gg.dL_dopacity = out(opac, {rows, 1});
    gg.dL_dmeans3D = out(means3D, {rows, 3});
    if (present(in.colors)) {
        gg.dL_dcolors = out(colors, {rows, 3});
    } else {
        gg.dL_dsh_dc = out(dc, {rows, 1, 3});
        if (present(in.sh_rest))
            gg.dL_dsh_rest = out(rest, {rows, in.sh_rest.numel() / std::max<int64_t>(in.means3D.size(0), 1) / 3, 3});
    }
    if (present(in.cov3D)) {
        gg.dL_dcov3D = out(cov, {rows, 6});
    } else {
        gg.dL_dscales = out(scales, {rows, 3});
        gg.dL_drotations = out(rots, {rows, 4});
    }
}
}  // namespace detail

namespace {
using namespace detail;  // check, Inputs, make_gaussians, make_settings, LeafGrads, present

struct AllocCtx {
    torch::Device device;
    std::vector<torch::Tensor> keep;
};

void* alloc_cb(void* ctx, size_t bytes) {
    auto* c = static_cast<AllocCtx*>(ctx);
    auto t = torch::empty({(int64_t)std::max<size_t>(bytes, 16)},
                          torch::TensorOptions().dtype(torch::kUInt8).device(c->device));
    c->keep.push_back(t);
    return t.data_ptr();
}

Frame forward_impl(const RasterCamera& cam, const RasterSettings& rs, const Inputs& in, bool aux = false,
                       bool inverse_depth = false) {
    const torch::Tensor& means3D = in.means3D;
    TORCH_CHECK(means3D.dim() == 2 && means3D.size(1) == 3, "means3D must be (P,3)");
    const int64_t P = means3D.size(0);
    auto dev = means3D.device();
    auto fopt = torch::TensorOptions().dtype(torch::kFloat32).device(dev);
    Frame r;
    r.color = torch::empty({3, cam.height, cam.width}, fopt);
    r.radii = torch::empty({P}, fopt.dtype(torch::kInt32));
    const gsr_camera c = cam.to_c();
    const gsr_gaussians g = make_gaussians(in, rs.sh_degree, rs.scale_modifier);
    gsr_raster_settings s = make_settings(rs);
    AllocCtx geom{dev, {}}, bin{dev, {}}, img{dev, {}};
    gsr_buffers b{};
    AllocCtx* ctxs[3] = {&geom, &bin, &img};  // one context per role
    const gsr_alloc_fn a0 = [](void* ctx, size_t n) { return alloc_cb(static_cast<AllocCtx**>(ctx)[0], n); };
    const gsr_alloc_fn a1 = [](void* ctx, size_t n) { return alloc_cb(static_cast<AllocCtx**>(ctx)[1], n); };
    const gsr_alloc_fn a2 = [](void* ctx, size_t n) { return alloc_cb(static_cast<AllocCtx**>(ctx)[2], n); };
    int32_t* const rad = P ? r.radii.data_ptr<int32_t>() : nullptr;
    if (aux) {  // the depth / alpha channels ride along (gsr.h gsr_forward_aux)
        r.depth = torch::empty({cam.height, cam.width}, fopt);
        r.alpha = torch::empty({cam.height, cam.width}, fopt);
        s.flags |= GSR_FLAG_AUX | (inverse_depth ? GSR_FLAG_INVDEPTH : 0u);
        const gsr_aux_out ao{r.depth.data_ptr<float>(), r.alpha.data_ptr<float>()};
        check(gsr_forward_aux(&c, &g, &s, r.color.data_ptr<float>(), rad, a0, a1, a2, (void*)ctxs, &b, current_stream(),
                              &ao),
              "gsr_forward_aux");
    } else {
        check(gsr_forward(&c, &g, &s, r.color.data_ptr<float>(), rad, a0, a1, a2, (void*)ctxs, &b, current_stream()),
              "gsr_forward");
    }
    r.geom = geom.keep.at(0);
    r.binning = bin.keep.empty() ? torch::Tensor() : bin.keep.at(0);
    r.image = img.keep.at(0);
    r.bufs = b;
    r.cam = c;
    r.settings = s;
    return r;
}

gsr_buffers buffers_of(const torch::Tensor& geom, const torch::Tensor& binning, const torch::Tensor& image,
                       int32_t K, int32_t cap, int32_t n_local, uint32_t layout) {
    gsr_buffers b{};
    b.layout = layout;  // the forward's layout word (gsr.h): the backward checks it
    b.geom = geom.data_ptr();
    b.binning = binning.defined() ? binning.data_ptr() : nullptr;
    b.image = image.data_ptr();
    b.num_rendered = K;
    b.capacity = cap;
    b.n_local = n_local;
    return b;
}

using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

// What both autograd Functions keep from forward to backward, and how backward gets it back
// (floats as doubles, which hold them exactly).
struct SavedFrame {
    RasterCamera cam;
    RasterSettings rs;
    int32_t K, cap, n_local;
    uint32_t layout;
    bool has_m2d;
};

void save_frame(AutogradContext* ctx, const RasterCamera& cam, const RasterSettings& rs, const Frame& r,
                const torch::Tensor& means2D) {
    auto doubles = [](const auto& a) { return std::vector<double>(a.begin(), a.end()); };
    // restore_frame reads the integers and the scalars back by position
    ctx->saved_data["ints"] = std::vector<int64_t>{r.bufs.num_rendered, r.bufs.capacity, r.bufs.n_local, r.bufs.layout,
                                                   present(means2D), cam.width, cam.height, rs.sh_degree, rs.tile_y0,
                                                   rs.tile_y1, rs.debug, rs.max_rendered, rs.antialiasing};
    ctx->saved_data["scalars"] = std::vector<double>{cam.tanfovx, cam.tanfovy, rs.scale_modifier};
    ctx->saved_data["cam_v"] = doubles(cam.viewmatrix);
    ctx->saved_data["cam_p"] = doubles(cam.projmatrix);
    ctx->saved_data["cam_c"] = doubles(cam.campos);
    ctx->saved_data["bg"] = doubles(rs.bg);
}

SavedFrame restore_frame(AutogradContext* ctx) {
    const auto n = ctx->saved_data["ints"].toIntVector();
    const auto x = ctx->saved_data["scalars"].toDoubleVector();
    auto floats = [&](const char* key, auto& dst) {
        const auto v = ctx->saved_data[key].toDoubleVector();
        for (size_t i = 0; i < dst.size(); ++i) dst[i] = (float)v[i];
    };
    SavedFrame f;
    f.K = (int32_t)n[0], f.cap = (int32_t)n[1], f.n_local = (int32_t)n[2], f.layout = (uint32_t)n[3];
    f.has_m2d = n[4] != 0;
    f.cam.width = (int)n[5], f.cam.height = (int)n[6];
    f.rs.sh_degree = (int)n[7], f.rs.tile_y0 = (int)n[8], f.rs.tile_y1 = (int)n[9];
    f.rs.debug = n[10] != 0, f.rs.max_rendered = (int)n[11], f.rs.antialiasing = n[12] != 0;
    f.cam.tanfovx = (float)x[0], f.cam.tanfovy = (float)x[1], f.rs.scale_modifier = (float)x[2];
    floats("cam_v", f.cam.viewmatrix);
    floats("cam_p", f.cam.projmatrix);
    floats("cam_c", f.cam.campos);
    floats("bg", f.rs.bg);
    return f;
}

// forward() of both autograd Functions: the render (inverse_depth != nullptr: with the depth and
// alpha channels), everything backward needs, and the outputs {color, (depth, alpha,) radii, K on
// the device, (K, capacity)}, all but the images non-differentiable.
variable_list forward_and_save(AutogradContext* ctx, const RasterCamera& cam, const RasterSettings& rs,
                               const bool* inverse_depth, const Inputs& in) {
    const bool aux = inverse_depth != nullptr;
    auto r = forward_impl(cam, rs, in, aux, aux && *inverse_depth);
    ctx->save_for_backward({in.means3D, in.sh_dc, in.sh_rest, in.colors, in.opac, in.scales, in.rots, in.cov3D, r.geom,
                            r.binning, r.image});
    save_frame(ctx, cam, rs, r, in.means2D);
    if (aux) ctx->saved_data["inverse_depth"] = *inverse_depth;
    auto kdev = r.k_device();
    auto kinfo = torch::tensor({r.bufs.num_rendered, r.bufs.capacity}, torch::kInt32);
    ctx->mark_non_differentiable({r.radii, kdev, kinfo});
    if (aux) return {r.color, r.depth, r.alpha, r.radii, kdev, kinfo};
    return {r.color, r.radii, kdev, kinfo};
}

// backward() of both: the gradients of (means3D, means2D, sh_dc, sh_rest, colors, opac, scales,
// rots, cov3D) from grad_out = {dL/dcolor} (gsr_backward), or with aux {dL/dcolor, dL/ddepth,
// dL/dalpha} (gsr_backward_aux): an output the loss does not use arrives as an undefined gradient
// and travels as NULL (= zero; the colour's as zeros).
variable_list backward_saved(AutogradContext* ctx, const variable_list& grad_out, bool aux) {
    const auto sv = ctx->get_saved_variables();  // forward_and_save's list
    const Inputs in{sv[0], {}, sv[1], sv[2], sv[3], sv[4], sv[5], sv[6], sv[7]};
    const SavedFrame f = restore_frame(ctx);
    auto dL_dcolor = aux && !grad_out[0].defined() ? torch::zeros({3, f.cam.height, f.cam.width}, in.means3D.options())
                                                   : grad_out[0].contiguous();
    const LeafGrads lg(in, in.means3D.size(0), /*want_conic=*/false);
    const gsr_camera c = f.cam.to_c();
    const gsr_gaussians g = make_gaussians(in, f.rs.sh_degree, f.rs.scale_modifier);
    gsr_raster_settings s = make_settings(f.rs);
    const gsr_buffers b = buffers_of(sv[8], sv[9], sv[10], f.K, f.cap, f.n_local, f.layout);
    AllocCtx scratch{in.means3D.device(), {}};
    if (aux) {
        torch::Tensor dL_ddepth, dL_dalpha;
        if (grad_out[1].defined()) dL_ddepth = grad_out[1].contiguous();
        if (grad_out[2].defined()) dL_dalpha = grad_out[2].contiguous();
        s.flags |= GSR_FLAG_AUX | (ctx->saved_data["inverse_depth"].toBool() ? GSR_FLAG_INVDEPTH : 0u);
        const gsr_aux_grads ag{dL_ddepth.defined() ? dL_ddepth.data_ptr<float>() : nullptr,
                               dL_dalpha.defined() ? dL_dalpha.data_ptr<float>() : nullptr};
        check(gsr_backward_aux(&c, &g, &s, &b, dL_dcolor.data_ptr<float>(), alloc_cb, &scratch, &lg.gg, current_stream(),
                               &ag),
              "gsr_backward_aux");
    } else {
        check(gsr_backward(&c, &g, &s, &b, dL_dcolor.data_ptr<float>(), alloc_cb, &scratch, &lg.gg, current_stream()),
              "gsr_backward");
    }
    // the canonical shapes, viewed as each input's own
    auto like = [](const torch::Tensor& g, const torch::Tensor& x) { return g.defined() ? g.view(x.sizes()) : g; };
    return {lg.means3D, f.has_m2d ? lg.means2D : torch::Tensor(), like(lg.dc, in.sh_dc), like(lg.rest, in.sh_rest),
            like(lg.colors, in.colors), like(lg.opac, in.opac), like(lg.scales, in.scales), like(lg.rots, in.rots),
            like(lg.cov, in.cov3D)};
}

class RasterizeGaussians : public torch::autograd::Function<RasterizeGaussians> {
   public:
    static variable_list forward(AutogradContext* ctx, const RasterCamera& cam, const RasterSettings& rs,
                                 torch::Tensor means3D, torch::Tensor means2D, torch::Tensor sh_dc,
                                 torch::Tensor sh_rest, torch::Tensor colors, torch::Tensor opac,
                                 torch::Tensor scales, torch::Tensor rots, torch::Tensor cov3D) {
        return forward_and_save(ctx, cam, rs, nullptr,
                                {means3D, means2D, sh_dc, sh_rest, colors, opac, scales, rots, cov3D});
    }

    static variable_list backward(AutogradContext* ctx, variable_list grad_out) {
        variable_list g = backward_saved(ctx, grad_out, false);
        g.insert(g.begin(), 2, torch::Tensor());  // cam, rs
        return g;
    }
};

// RasterizeGaussians with the depth and alpha outputs (gsr_forward_aux / gsr_backward_aux): one
// forward, one backward for a loss over colour, depth and alpha.
class RasterizeGaussiansAux : public torch::autograd::Function<RasterizeGaussiansAux> {
   public:
    static variable_list forward(AutogradContext* ctx, const RasterCamera& cam, const RasterSettings& rs,
                                 bool inverse_depth, torch::Tensor means3D, torch::Tensor means2D,
                                 torch::Tensor sh_dc, torch::Tensor sh_rest, torch::Tensor colors, torch::Tensor opac,
                                 torch::Tensor scales, torch::Tensor rots, torch::Tensor cov3D) {
        return forward_and_save(ctx, cam, rs, &inverse_depth,
                                {means3D, means2D, sh_dc, sh_rest, colors, opac, scales, rots, cov3D});
    }

    static variable_list backward(AutogradContext* ctx, variable_list grad_out) {
        variable_list g = backward_saved(ctx, grad_out, true);
        g.insert(g.begin(), 3, torch::Tensor());  // cam, rs, inverse_depth
        return g;
    }
};

// Both rasterize_gaussians entry points (inverse_depth != nullptr: the aux Function).  Absent
// optional inputs go in as defined 0-element tensors (see present()).
std::vector<torch::Tensor> rasterize(const RasterCamera& cam, const RasterSettings& rs, const bool* inverse_depth,
                                     Inputs in) {
    auto none = torch::empty({0}, in.means3D.options());
    for (torch::Tensor* t : {&in.means2D, &in.sh_dc, &in.sh_rest, &in.colors, &in.scales, &in.rots, &in.cov3D})
        if (!t->defined()) *t = none;
    if (inverse_depth)
        return RasterizeGaussiansAux::apply(cam, rs, *inverse_depth, in.means3D, in.means2D, in.sh_dc, in.sh_rest,
                                            in.colors, in.opac, in.scales, in.rots, in.cov3D);
    return RasterizeGaussians::apply(cam, rs, in.means3D, in.means2D, in.sh_dc, in.sh_rest, in.colors, in.opac,
                                     in.scales, in.rots, in.cov3D);
}

}  // namespace

namespace detail {
torch::Tensor Frame::k_device() const {
    const void* p = gsr_view(&cam, bufs.n_local, &bufs, GSR_VIEW_COUNTS);
    TORCH_CHECK(p != nullptr, "gsr_view(COUNTS) returned NULL");
    const int64_t off = static_cast<const uint8_t*>(p) - static_cast<const uint8_t*>(image.data_ptr());
    TORCH_CHECK(off >= 0 && off + 4 <= image.numel(), "K counter outside the image buffer");
    return image.narrow(0, off, 4).view(torch::kInt32).clone();  // async device copy
}

Frame forward(const RasterCamera& cam, const RasterSettings& rs, const Inputs& in) {
    return forward_impl(cam, rs, in);
}

void backward(const Frame& f, const RasterSettings& rs, const Inputs& in, const torch::Tensor& dL_dcolor,
              const gsr_grads& grads) {
    const gsr_gaussians g = make_gaussians(in, rs.sh_degree, rs.scale_modifier);
    TORCH_CHECK(dL_dcolor.is_contiguous() && dL_dcolor.numel() == 3LL * f.cam.width * f.cam.height,
                "dL_dcolor must be a contiguous (3,H,W) tensor");
    AllocCtx scratch{in.means3D.device(), {}};
    check(gsr_backward(&f.cam, &g, &f.settings, &f.bufs, dL_dcolor.data_ptr<float>(), alloc_cb, &scratch, &grads,
                       current_stream()),
          "gsr_backward");
}
}  // namespace detail

int read_num_rendered(const RenderOutput& out) {
    const int k = out.num_rendered_device.item<int32_t>();  // waits for the render's stream
    if (k > out.capacity)
        throw std::overflow_error("num_rendered " + std::to_string(k) + " exceeded the binning capacity " +
                                  std::to_string(out.capacity) + " (GSR_ERR_OVERFLOW): re-render with a larger bound");
    return k;
}

std::array<float, 3> background(const torch::Tensor& bg) {
    TORCH_CHECK(bg.numel() == 3, "background must have 3 values");
    auto h = bg.to(torch::kCPU, torch::kFloat32).contiguous();
    return {h.data_ptr<float>()[0], h.data_ptr<float>()[1], h.data_ptr<float>()[2]};
}

BinningCapacity::BinningCapacity(double headroom, int ring, bool strict) : headroom_(headroom), strict_(strict) {
    const bool pin = torch::cuda::is_available();
    for (int i = 0; i < ring; ++i) {
        slots_.push_back(torch::zeros({1}, torch::TensorOptions().dtype(torch::kInt32).pinned_memory(pin)));
        events_.push_back(new c10::Event(c10::DeviceType::CUDA));  // torch's event: one HIP runtime
    }
}

BinningCapacity::~BinningCapacity() {
    for (void* e : events_) delete static_cast<c10::Event*>(e);
}

void BinningCapacity::grow() { cap_ = (int)(((int64_t)(k_max_ * headroom_) + 65536 + 4095) / 4096 * 4096); }

int BinningCapacity::bound() {
    poll(false);
    return cap_;
}

void BinningCapacity::reset() {
    pending_.clear();
    cap_ = 0;
    k_max_ = 0;
}

void BinningCapacity::observe(const RenderOutput& out) { observe(out.num_rendered_device, out.num_rendered); }

void BinningCapacity::observe(const torch::Tensor& k_device, int host_k) {
    if (cap_ == 0) {  // an exactly sized render: its K was read back by the forward
        ++exact_reads_;
        k_max_ = std::max<int64_t>(k_max_, host_k);
        grow();
        return;
    }
    if (pending_.size() == slots_.size()) poll(true);  // ring full: wait for the oldest
    const int slot = next_;
    next_ = (next_ + 1) % (int)slots_.size();
    slots_[slot].copy_(k_device, /*non_blocking=*/true);
    static_cast<c10::Event*>(events_[slot])->record(at::hip::getCurrentHIPStreamMasqueradingAsCUDA().unwrap());
    pending_.push_back({slot, events_[slot], cap_});
}

void BinningCapacity::sync() {
    while (!pending_.empty()) poll(true);
}

void BinningCapacity::poll(bool wait_one) {
    bool waited = false;
    while (!pending_.empty()) {
        auto* e = static_cast<c10::Event*>(pending_.front().event);
        if (wait_one && !waited) {
            e->synchronize();
            waited = true;
        } else if (!e->query()) {
            break;
        }
        const Pending p = pending_.front();
        pending_.erase(pending_.begin());
        const int64_t k = slots_[p.slot].data_ptr<int32_t>()[0];
        if (k > p.cap) {  // that render was truncated (its statistics / Adam step skipped on the device)
            if (overflows_ == 0)
                std::fprintf(stderr, "[gsr] BinningCapacity: a render's K = %lld exceeded its bound %d; that "
                             "iteration's update was skipped on the device, renders are sized exactly again\n",
                             (long long)k, p.cap);
            ++overflows_;
            k_max_ = std::max(k_max_, k);
            pending_.clear();
            cap_ = 0;  // the next render is sized exactly
            if (strict_)
                throw std::overflow_error("a render's K = " + std::to_string(k) + " exceeded its bound " +
                                          std::to_string(p.cap));
            return;
        }
        if (k > k_max_) {
            k_max_ = k;
            if (k * 1.2 > cap_) grow();
        }
    }
}

RasterCamera RasterCamera::from_tensors(int width, int height, double FoVx, double FoVy,
                                        const torch::Tensor& wv, const torch::Tensor& fp,
                                        const torch::Tensor& cc) {
    RasterCamera c;
    c.width = width;
    c.height = height;
    c.tanfovx = (float)std::tan(FoVx * 0.5);
    c.tanfovy = (float)std::tan(FoVy * 0.5);
    auto v = wv.to(torch::kCPU, torch::kFloat32).contiguous();
    auto p = fp.to(torch::kCPU, torch::kFloat32).contiguous();
    auto o = cc.to(torch::kCPU, torch::kFloat32).contiguous();
    for (int i = 0; i < 16; ++i) c.viewmatrix[i] = v.data_ptr<float>()[i], c.projmatrix[i] = p.data_ptr<float>()[i];
    for (int i = 0; i < 3; ++i) c.campos[i] = o.data_ptr<float>()[i];
    return c;
}

gsr_camera RasterCamera::to_c() const {
    gsr_camera c{};
    c.width = width;
    c.height = height;
    c.tanfovx = tanfovx;
    c.tanfovy = tanfovy;
    for (int i = 0; i < 16; ++i) c.viewmatrix[i] = viewmatrix[i], c.projmatrix[i] = projmatrix[i];
    for (int i = 0; i < 3; ++i) c.campos[i] = campos[i];
    return c;
}

std::vector<torch::Tensor> rasterize_gaussians(const RasterCamera& cam, const RasterSettings& rs,
                                               const torch::Tensor& means3D, const torch::Tensor& means2D,
                                               const torch::Tensor& sh_dc, const torch::Tensor& sh_rest,
                                               const torch::Tensor& colors, const torch::Tensor& opac,
                                               const torch::Tensor& scales, const torch::Tensor& rots,
                                               const torch::Tensor& cov3D) {
    return rasterize(cam, rs, nullptr, {means3D, means2D, sh_dc, sh_rest, colors, opac, scales, rots, cov3D});
}

std::vector<torch::Tensor> rasterize_gaussians_aux(const RasterCamera& cam, const RasterSettings& rs,
                                                   bool inverse_depth, const torch::Tensor& means3D,
                                                   const torch::Tensor& means2D, const torch::Tensor& sh_dc,
                                                   const torch::Tensor& sh_rest, const torch::Tensor& colors,
                                                   const torch::Tensor& opac, const torch::Tensor& scales,
                                                   const torch::Tensor& rots, const torch::Tensor& cov3D) {
    return rasterize(cam, rs, &inverse_depth, {means3D, means2D, sh_dc, sh_rest, colors, opac, scales, rots, cov3D});
}

torch::Tensor eval_sh_colors(int D, const torch::Tensor& sh, const torch::Tensor& dirs) {
    // same basis and constants as the kernels
    const double C0 = 0.28209479177387814, C1 = 0.4886025119029199;
    const double C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792,
                          0.5462742152960396};
    const double C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                          -0.4570457994644658, 1.445305721320277, -0.5900435899266435};
    using torch::indexing::Slice;
    auto c = [&](int k) { return sh.index({Slice(), k}); };
    auto res = C0 * c(0);
    if (D > 0) {
        auto x = dirs.index({Slice(), Slice(0, 1)}), y = dirs.index({Slice(), Slice(1, 2)}),
             z = dirs.index({Slice(), Slice(2, 3)});
        res = res - C1 * y * c(1) + C1 * z * c(2) - C1 * x * c(3);
        if (D > 1) {
            auto xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            res = res + C2[0] * xy * c(4) + C2[1] * yz * c(5) + C2[2] * (2.0 * zz - xx - yy) * c(6) +
                  C2[3] * xz * c(7) + C2[4] * (xx - yy) * c(8);
            if (D > 2) {
                res = res + C3[0] * y * (3 * xx - yy) * c(9) + C3[1] * xy * z * c(10) +
                      C3[2] * y * (4 * zz - xx - yy) * c(11) + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * c(12) +
                      C3[4] * x * (4 * zz - xx - yy) * c(13) + C3[5] * z * (xx - yy) * c(14) +
                      C3[6] * x * (xx - 3 * yy) * c(15);
            }
        }
    }
    return torch::clamp_min(res + 0.5, 0.0);
}

}  // namespace gsr
