"""MI355X-native volumetric feature aggregation (the un-projection hot path of MultiviewHMR).

Public surface mirrors the reference modules it replaces:

    multiviewhmr_amd.aggregation   <->  models/aggregation.py   (unprojection, VolumeGenerator, build_volume_generator)
    multiviewhmr_amd.multiview     <->  utils/multiview.py      (Camera, projection helpers, DLT triangulation)
    multiviewhmr_amd.volumetric    <->  utils/volumetric.py     (Cuboid3D, get_rotation_matrix, rotate_coord_volume)

and, beyond them, multiviewhmr_amd.softargmax: the volumetric 3-D soft-argmax that turns a heat volume back into keypoints
(soft_argmax_3d, soft_argmax_3d_cuboid), and multiviewhmr_amd.volsample: reading a volume back at world points (sample_volume_cuboid,
volumetric_cross_entropy), and multiviewhmr_amd.peaks: 3-D non-maximum suppression with top-K, the proposals a multi-person pipeline places
its fine volumes at (volume_peaks, volume_peaks_cuboid, peak_proposals), and multiviewhmr_amd.volproject: rendering a volume into the cameras
by ray-marching (camera_rays, project_volume_cuboid).

The compute lives in lib/libmvhmr_unproject.so (hand-written HIP for gfx950 behind the C ABI of
include/mvhmr_unproject.h); there is no CPU or PyTorch fallback -- importing is cheap, calling
`unprojection` without the built library or without a HIP device raises.
"""
__version__ = "0.1.0"

from . import aggregation, multiview, peaks, softargmax, volproject, volsample, volumetric  # noqa: F401
from .aggregation import VolumeGenerator, build_volume_generator, unprojection  # noqa: F401
from .softargmax import soft_argmax_3d, soft_argmax_3d_cuboid  # noqa: F401
from .peaks import peak_proposals, volume_peaks, volume_peaks_cuboid  # noqa: F401
from .volsample import sample_volume_cuboid, volumetric_cross_entropy  # noqa: F401
from .volproject import camera_rays, project_volume_cuboid  # noqa: F401
