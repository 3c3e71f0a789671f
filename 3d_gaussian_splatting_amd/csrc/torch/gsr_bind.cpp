// gsr_bind.cpp -- the Python binding (_gsr_torch) of the libtorch layer: the rasterizer entry
// points of gsr_render.h, the depth loss of gsr_trainer.h and the multi-GPU step of gsr_shard.h
// (the benchmark's multi-GPU path).
// The only file of the layer that includes pybind11; a C++ executable links the others without it.
#include <pybind11/stl.h>
#include <torch/extension.h>
#include <torch/csrc/distributed/c10d/Store.hpp>

#include "gsr_render.h"
#include "gsr_shard.h"
#include "gsr_trainer.h"

namespace py = pybind11;

static gsr::RasterCamera cam_from_py(int w, int h, float tx, float ty, const std::vector<float>& v,
                                     const std::vector<float>& p, const std::vector<float>& c) {
    TORCH_CHECK(v.size() == 16 && p.size() == 16 && c.size() == 3, "bad camera arrays");
    gsr::RasterCamera cam;
    cam.width = w;
    cam.height = h;
    cam.tanfovx = tx;
    cam.tanfovy = ty;
    for (int i = 0; i < 16; ++i) cam.viewmatrix[i] = v[i], cam.projmatrix[i] = p[i];
    for (int i = 0; i < 3; ++i) cam.campos[i] = c[i];
    return cam;
}

static gsr::RasterSettings settings_from_py(const std::vector<float>& bg, float smod, int D, int ty0, int ty1,
                                            bool debug, int max_rendered, bool antialiasing) {
    gsr::RasterSettings rs;
    rs.antialiasing = antialiasing;
    rs.max_rendered = max_rendered;
    for (int i = 0; i < 3; ++i) rs.bg[i] = bg.at(i);
    rs.scale_modifier = smod;
    rs.sh_degree = D;
    rs.tile_y0 = ty0;
    rs.tile_y1 = ty1;
    rs.debug = debug;
    return rs;
}

using OptTensor = c10::optional<torch::Tensor>;
static torch::Tensor opt(const OptTensor& t) { return t.has_value() ? *t : torch::Tensor(); }

namespace gsr {
static void bind_shard(py::module& m) {
    static py::exception<ShardOverflowError> ovf(m, "ShardOverflowError", PyExc_OverflowError);
    py::register_exception_translator([](std::exception_ptr p) {
        try {
            if (p) std::rethrow_exception(p);
        } catch (const ShardOverflowError& e) {
            py::object cls = py::reinterpret_borrow<py::object>(ovf.ptr());
            py::object err = cls(e.what());
            err.attr("step") = e.step;
            err.attr("rank") = e.rank;
            err.attr("counts") = e.counts;
            err.attr("pair_cap") = e.pair_cap;
            err.attr("band_k") = e.band_k;
            err.attr("capacity") = e.capacity;
            PyErr_SetObject(ovf.ptr(), err.ptr());
        }
    });
    py::class_<Exchange>(m, "Exchange")
        .def_property_readonly("rank", &Exchange::rank)
        .def_property_readonly("world", &Exchange::world)
        .def_property_readonly("name", &Exchange::name)
        .def_property_readonly("comm_world", &Exchange::comm_world)
        .def_property_readonly("capturable", &Exchange::capturable);
    m.def(
        "plan_from_stats",
        [](const std::vector<int64_t>& inst, const std::vector<std::vector<int64_t>>& starts,
           const std::vector<std::vector<int64_t>>& ends, int world) {
            const StatsPlan sp = plan_from_stats(inst, starts, ends, world);
            return py::make_tuple(sp.rows, sp.max_splats, sp.band_k);
        },
        py::arg("inst"), py::arg("starts"), py::arg("ends"), py::arg("world"));
    m.def("rccl_unique_id", []() {
        auto v = rccl_unique_id();
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
    });
    m.def(
        "rccl_exchange",
        [](py::bytes id, int rank, int world) {
            const std::string b = id;
            return rccl_exchange(std::vector<uint8_t>(b.begin(), b.end()), rank, world);
        },
        py::arg("unique_id"), py::arg("rank"), py::arg("world"));
    // host-staged exchange through a torch.distributed Store (e.g. the default group's,
    // torch.distributed.distributed_c10d._get_default_store()): ranks may share a GPU (rehearsal)
    m.def(
        "store_exchange",
        [](const c10::intrusive_ptr<c10d::Store>& store, int rank, int world) {
            std::shared_ptr<c10d::Store> s(store.get(), [keep = store](c10d::Store*) mutable { keep.reset(); });
            py::gil_scoped_release nogil;  // the join waits for the other ranks
            return store_exchange(std::move(s), rank, world);
        },
        py::arg("store"), py::arg("rank"), py::arg("world"));
    py::class_<LocalGroup, std::shared_ptr<LocalGroup>>(m, "LocalGroup")
        .def(py::init([](int world) { return local_group(world); }), py::arg("world"))
        .def_property_readonly("world", &LocalGroup::world);
    m.def("local_exchange", &local_exchange, py::arg("group"), py::arg("rank"), py::keep_alive<0, 1>());
    m.def("local_exchange_set_replay", &local_exchange_set_replay, py::arg("exchange"), py::arg("on"),
          py::arg("copies") = true);
    m.def(
        "run_ranks_plan", [](const std::vector<ShardStep*>& steps) { run_ranks_plan(steps); }, py::arg("steps"),
        py::call_guard<py::gil_scoped_release>());
    m.def(
        "run_ranks_steps",
        [](const std::vector<ShardStep*>& steps, const torch::Tensor& dpix, int n) { run_ranks_steps(steps, dpix, n); },
        py::arg("steps"), py::arg("dL_dpix"), py::arg("n"), py::call_guard<py::gil_scoped_release>());
    py::class_<ShardStep>(m, "ShardStep")
        .def(py::init([](Exchange& ex, const RasterCamera& cam, py::dict inputs, int sh_degree,
                         std::array<float, 3> bg, double headroom, bool graph, int lag) {
                 ShardInputs in;
                 auto get = [&](const char* k) {
                     return inputs.contains(k) && !inputs[k].is_none() ? inputs[k].cast<torch::Tensor>()
                                                                        : torch::Tensor();
                 };
                 in.means3D = get("means3D");
                 in.opacities = get("opacities");
                 in.scales = get("scales");
                 in.rotations = get("rotations");
                 in.sh_dc = get("sh_dc");
                 in.sh_rest = get("sh_rest");
                 in.colors_precomp = get("colors_precomp");
                 in.cov3D_precomp = get("cov3D_precomp");
                 in.sh_degree = sh_degree;
                 return std::make_unique<ShardStep>(ex, cam, in, bg, headroom, graph, lag);
             }),
             py::arg("exchange"), py::arg("cam"), py::arg("inputs"), py::arg("sh_degree"),
             py::arg("bg") = std::array<float, 3>{0.f, 0.f, 0.f}, py::arg("headroom") = 1.25,
             py::arg("graph") = true, py::arg("lag") = 2, py::keep_alive<1, 2>())
        .def("plan", &ShardStep::plan, py::call_guard<py::gil_scoped_release>())
        .def(
            "step",
            [](ShardStep& s, const torch::Tensor& dpix) {
                ShardStep::Result r;
                {
                    py::gil_scoped_release nogil;
                    r = s.step(dpix);
                }
                return py::make_tuple(r.image, r.grads, r.radii);
            },
            py::arg("dL_dpix"))
        .def("check", &ShardStep::check, py::call_guard<py::gil_scoped_release>())
        .def("set_pair_cap", &ShardStep::set_pair_cap)
        .def("set_camera", &ShardStep::set_camera, py::arg("cam"))
        .def("set_rebalance_every", &ShardStep::set_rebalance_every, py::arg("m"))
        .def_property_readonly("replans", &ShardStep::replans)
        .def("set_live_replan", &ShardStep::set_live_replan, py::arg("on"))
        .def("set_graph", &ShardStep::set_graph, py::arg("on"))
        .def_property_readonly("live_replans", &ShardStep::live_replans)
        .def("band_num_rendered", &ShardStep::band_num_rendered)
        .def_property_readonly("rows", &ShardStep::rows)
        .def_property_readonly("pair_cap", &ShardStep::pair_cap)
        .def_property_readonly("capacity", &ShardStep::capacity)
        .def_property_readonly("band_instances", &ShardStep::band_instances)
        .def_property_readonly("g0", &ShardStep::g0)
        .def_property_readonly("g1", &ShardStep::g1)
        .def_property_readonly("exchange_world", &ShardStep::exchange_world)
        .def_property_readonly("overflow_guard", &ShardStep::overflow_guard)
        .def_property_readonly("exchange_name", &ShardStep::exchange_name)
        .def_property_readonly("graph_active", &ShardStep::graph_active)
        .def_property_readonly("steps", &ShardStep::steps);
}
}  // namespace gsr

PYBIND11_MODULE(_gsr_torch, m) {
    m.doc() = "libtorch RasterizeGaussians over the gsr C ABI (libgsr_hip.so)";
    py::class_<gsr::RasterCamera>(m, "RasterCamera")
        .def(py::init(&cam_from_py), py::arg("width"), py::arg("height"), py::arg("tanfovx"),
             py::arg("tanfovy"), py::arg("viewmatrix"), py::arg("projmatrix"), py::arg("campos"))
        .def_readonly("width", &gsr::RasterCamera::width)
        .def_readonly("height", &gsr::RasterCamera::height)
        .def_readonly("tanfovx", &gsr::RasterCamera::tanfovx)
        .def_readonly("tanfovy", &gsr::RasterCamera::tanfovy)
        .def_readonly("viewmatrix", &gsr::RasterCamera::viewmatrix)
        .def_readonly("projmatrix", &gsr::RasterCamera::projmatrix)
        .def_readonly("campos", &gsr::RasterCamera::campos);
    py::class_<gsr::RasterSettings>(m, "RasterSettings")
        .def(py::init(&settings_from_py), py::arg("bg"), py::arg("scale_modifier") = 1.0f,
             py::arg("sh_degree") = 0, py::arg("tile_y0") = 0, py::arg("tile_y1") = INT32_MAX,
             py::arg("debug") = false, py::arg("max_rendered") = 0, py::arg("antialiasing") = false)
        .def_readonly("antialiasing", &gsr::RasterSettings::antialiasing);
    m.def(
        "rasterize_gaussians",
        [](const gsr::RasterCamera& cam, const gsr::RasterSettings& rs, torch::Tensor means3D, torch::Tensor means2D,
           OptTensor sh_dc, OptTensor sh_rest, OptTensor colors, torch::Tensor opac, OptTensor scales, OptTensor rots,
           OptTensor cov3D) {
            auto r = gsr::rasterize_gaussians(cam, rs, means3D, means2D, opt(sh_dc), opt(sh_rest), opt(colors), opac,
                                              opt(scales), opt(rots), opt(cov3D));
            return py::make_tuple(r[0], r[1]);
        },
        py::arg("cam"), py::arg("settings"), py::arg("means3D"), py::arg("means2D"), py::arg("sh_dc"),
        py::arg("sh_rest"), py::arg("colors_precomp"), py::arg("opacities"), py::arg("scales"),
        py::arg("rotations"), py::arg("cov3D_precomp"));
    m.def(
        "rasterize_gaussians_aux",
        [](const gsr::RasterCamera& cam, const gsr::RasterSettings& rs, bool inverse_depth, torch::Tensor means3D,
           torch::Tensor means2D, OptTensor sh_dc, OptTensor sh_rest, OptTensor colors, torch::Tensor opac,
           OptTensor scales, OptTensor rots, OptTensor cov3D) {
            auto r = gsr::rasterize_gaussians_aux(cam, rs, inverse_depth, means3D, means2D, opt(sh_dc), opt(sh_rest),
                                                  opt(colors), opac, opt(scales), opt(rots), opt(cov3D));
            return py::make_tuple(r[0], r[1], r[2], r[3]);
        },
        py::arg("cam"), py::arg("settings"), py::arg("inverse_depth"), py::arg("means3D"), py::arg("means2D"),
        py::arg("sh_dc"), py::arg("sh_rest"), py::arg("colors_precomp"), py::arg("opacities"), py::arg("scales"),
        py::arg("rotations"), py::arg("cov3D_precomp"));
    m.def(
        "depth_loss",
        [](torch::Tensor depth, OptTensor alpha, torch::Tensor target, OptTensor mask, double weight, int mode,
           double alpha_min) {
            torch::Tensor stats;
            auto loss = gsr::depth_loss(depth, opt(alpha), target, opt(mask), weight, mode, alpha_min, &stats);
            return py::make_tuple(loss, stats);
        },
        py::arg("depth"), py::arg("alpha"), py::arg("target"), py::arg("mask"), py::arg("weight") = 1.0,
        py::arg("mode") = GSR_DEPTH_RAW, py::arg("alpha_min") = 0.5);
    m.def(
        "apply_exposure",
        [](torch::Tensor image, torch::Tensor exposure, bool clamp) { return gsr::apply_exposure(image, exposure, clamp); },
        py::arg("image"), py::arg("exposure"), py::arg("clamp") = false);
    m.def("eval_sh_colors", &gsr::eval_sh_colors);
    m.def(
        "camera_from_tensors",
        [](int w, int h, double fovx, double fovy, torch::Tensor wv, torch::Tensor fp, torch::Tensor cc) {
            return gsr::RasterCamera::from_tensors(w, h, fovx, fovy, wv, fp, cc);
        },
        py::arg("width"), py::arg("height"), py::arg("FoVx"), py::arg("FoVy"), py::arg("world_view_transform"),
        py::arg("full_proj_transform"), py::arg("camera_center"));
    m.def("abi_version", []() { return gsr_abi_version(); });
    gsr::bind_shard(m);
}
