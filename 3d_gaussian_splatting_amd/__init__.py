"""gsr -- MI355X-native differentiable 3D Gaussian splat rasterizer.

Drop-in for the render()/backward() hot path of seiya-kumada/3d_gaussian_splatting
(insertion point src/utils/train_utils.cpp:137-144).  Layers:

  include/gsr/gsr.h              C ABI (plain pointers, sizes, hipStream_t)
  csrc/*.hip -> lib/libgsr_hip.so  hand-written CDNA4 kernels behind that ABI
  csrc/torch/ -> lib/_gsr_torch*.so and the C++ executables: the libtorch layer
    gsr_render.h, gsr_torch.cpp      render(), the autograd Functions, the tensor-to-ABI glue
    gsr_trainer.{h,cpp}              the training step (executables only)
    gsr_plan / gsr_exchange / gsr_shard .{h,cpp}   the multi-GPU step: partition arithmetic
                                     (standard library only), transports, ShardStep
    gsr_bind.cpp                     the Python binding (extension only)
  rasterizer.py                   Python mirror of the same surface (tests / bench)

Importing the package does not touch the GPU.  ``native`` loads the shared libraries
and raises if they are missing: there is no CPU fallback in the product path.
"""
from . import graphics, scene  # noqa: F401

__all__ = ["graphics", "scene"]
