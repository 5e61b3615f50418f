"""The camera models and the Camera of the Python side, once: `scene` and `workspace` derive their tables and their
camera class from here. The same facts as include/colmap_amd/camera_models.hpp (reference sensor/models.h);
tests/test_camera_models.py holds both against one fixture."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple, Optional

import numpy as np


class CameraModel(NamedTuple):
    name: str
    num_params: int
    focal_length_idxs: List[int]
    principal_point_idxs: List[int]
    extra_params_idxs: List[int]
    is_fisheye: bool = False
    is_spherical: bool = False


# index = colmap::CameraModelId; the parameters are (f | fx fy) cx cy extra...
MODELS = [
    CameraModel("SIMPLE_PINHOLE", 3, [0], [1, 2], []),
    CameraModel("PINHOLE", 4, [0, 1], [2, 3], []),
    CameraModel("SIMPLE_RADIAL", 4, [0], [1, 2], [3]),
    CameraModel("RADIAL", 5, [0], [1, 2], [3, 4]),
    CameraModel("OPENCV", 8, [0, 1], [2, 3], [4, 5, 6, 7]),
    CameraModel("OPENCV_FISHEYE", 8, [0, 1], [2, 3], [4, 5, 6, 7], is_fisheye=True),
    CameraModel("FULL_OPENCV", 12, [0, 1], [2, 3], list(range(4, 12))),
    CameraModel("FOV", 5, [0, 1], [2, 3], [4]),
    CameraModel("SIMPLE_RADIAL_FISHEYE", 4, [0], [1, 2], [3], is_fisheye=True),
    CameraModel("RADIAL_FISHEYE", 5, [0], [1, 2], [3, 4], is_fisheye=True),
    CameraModel("THIN_PRISM_FISHEYE", 12, [0, 1], [2, 3], list(range(4, 12)), is_fisheye=True),
    CameraModel("RAD_TAN_THIN_PRISM_FISHEYE", 16, [0, 1], [2, 3], list(range(4, 16)), is_fisheye=True),
    CameraModel("SIMPLE_DIVISION", 4, [0], [1, 2], [3]),
    CameraModel("DIVISION", 5, [0, 1], [2, 3], [4]),
    CameraModel("SIMPLE_FISHEYE", 3, [0], [1, 2], [], is_fisheye=True),
    CameraModel("FISHEYE", 4, [0, 1], [2, 3], [], is_fisheye=True),
    CameraModel("EUCM", 6, [0, 1], [2, 3], [4, 5]),
    # (width, height) are metadata parameters, never refined (MetaDataParamsIdxs, models.h:2839-2842)
    CameraModel("EQUIRECTANGULAR", 2, [], [], [], is_spherical=True),
]


def model(model_id: int) -> Optional[CameraModel]:
    """The model of an id; None for an id that is not a model."""
    return MODELS[model_id] if 0 <= model_id < len(MODELS) else None


@dataclass
class Camera:
    """scene/camera.h"""
    camera_id: int
    model_id: int
    width: int
    height: int
    params: np.ndarray  # float64

    def CalibrationMatrix(self) -> np.ndarray:
        """Camera::CalibrationMatrix (scene/camera.cc:63-72)."""
        m = model(self.model_id)
        if m is None:
            raise KeyError(self.model_id)
        if m.is_spherical:
            raise ValueError(f"{m.name} cameras have no calibration matrix")
        K = np.eye(3)
        K[0, 0], K[1, 1] = self.params[m.focal_length_idxs[0]], self.params[m.focal_length_idxs[-1]]
        K[0, 2], K[1, 2] = self.params[m.principal_point_idxs[0]], self.params[m.principal_point_idxs[1]]
        return K
