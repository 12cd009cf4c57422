"""libsrcnn_amd -- MI355X-native SRCNN Y-channel path behind the rageworx/libsrcnn interface.

The product is libsrcnn_amd/lib/libsrcnn_amd.so (hand-written gfx950 kernels + C ABI
include/srcnn_amd.h + the C++ drop-in symbols ProcessSRCNN / ConfigureFilterSRCNN).  This package
is only the ctypes binding used by tests/, bench.py and __graft_entry__.py; it mirrors the
reference's two public calls (src/libsrcnn.h:46-54) and exposes the planar-float Y entry points.

There is no CPU compute path here: if the shared object is missing, or no gfx950 device is
visible, calls raise.

This file only re-exports.  The code, one module per family of headers under include/:
  abi         constants, structs and the ONE table of exported C functions; the *_SYMBOLS lists and the argtypes come from it
  core        lib(), errors, contexts / modes / profile, DeviceBuffer / Stream / Event / PinnedArray, the marshalling helpers
  ypath       the Y path: frame, band, batch, stream, stages, rect, rect list, delta
  yuv         planar / semi-planar YUV: frame, rect, rect list
  yuv_packed  packed YUV: frame, rect, rect list
  rgb         RGB(A): frame, rect, rect list, delta; process_u8, ProcessJob and the two drop-in names
  rgb_torch   the RGB(A) calls on torch tensors (torch is imported by the calls only)
"""
import ctypes as C     # noqa: F401  (C, np and os have always been attributes of the package)
import os              # noqa: F401

import numpy as np     # noqa: F401

from . import abi, core, rgb, rgb_torch, ypath, yuv, yuv_packed
from .abi import *          # noqa: F401,F403
from .core import *         # noqa: F401,F403
from .rgb import *          # noqa: F401,F403
from .rgb_torch import *    # noqa: F401,F403
from .ypath import *        # noqa: F401,F403
from .yuv import *          # noqa: F401,F403
from .yuv_packed import *   # noqa: F401,F403

__all__ = abi.__all__ + core.__all__ + ypath.__all__ + yuv.__all__ + yuv_packed.__all__ + rgb.__all__ + rgb_torch.__all__
