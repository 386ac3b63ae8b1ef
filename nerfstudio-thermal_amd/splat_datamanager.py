"""Full-image datamanager of the splat path: the counterpart of the reference's FullImageDatamanager
(nerfstudio/data/datamanagers/full_images_datamanager.py) for this package's dataparser and splat.PinholeCamera.

At construction every train and eval frame is loaded, moved to the device and -- the rasteriser being strictly pinhole -- undistorted once with
its own camera and coefficients (cache_images / _undistort_image, :132-225 and :351-386; here splat.undistort_image: tn_image_undistort, and
splat.undistorted_camera for the intrinsics that go with the frame).  RGB and thermal frames differ in size and distortion; each keeps its own.
The cache is uint8 by default (the reference's cache_images_type; ThermalSplatfactoModel.get_gt_img converts) and stays on the device.  Training
and evaluation get whole frames as (camera, batch), batch = {"image", "is_thermal", "image_idx"}, drawn so that every camera is seen once before
any is seen again (:301-348).  The draws come from a random.Random(seed) the datamanager owns, not from the global generator, so two runs with
one seed see one order.  A batch is a new dict over the cached tensor (the reference deep-copies the frame on every step; nothing here writes
to a batch's image).  Masks, depth images and fisheye cameras are not built."""
from __future__ import annotations

import dataclasses
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from .dataparser import DataparserOutputs, ThermalNerfDataParserConfig, load_image_float32, load_image_uint8
from .splat import PinholeCamera, undistort_image

Batch = Dict[str, object]


@dataclass
class ThermalFullImageDatamanagerConfig:
    dataparser: ThermalNerfDataParserConfig = field(default_factory=ThermalNerfDataParserConfig)
    cache_images_type: str = "uint8"  # "uint8" | "float32"
    undistort: bool = True  # False: the raw frames with the parser's intrinsics, distortion dropped
    eval_split: str = "val"
    seed: int = 0

    def __post_init__(self):
        if self.cache_images_type not in ("uint8", "float32"):
            raise ValueError(f"cache_images_type = {self.cache_images_type!r} (\"uint8\" or \"float32\")")

    def setup(self, device="cuda") -> "ThermalFullImageDatamanager":
        return ThermalFullImageDatamanager(self, device=device)


def parsed_camera(outputs: DataparserOutputs, i: int) -> PinholeCamera:
    """Camera i of a dataparser split as the rasteriser's PinholeCamera (the distortion is outputs.cameras["distortion"][i])."""
    cams = outputs.cameras
    return PinholeCamera(cams["c2w"][i].float(), float(cams["fx"][i]), float(cams["fy"][i]), float(cams["cx"][i]), float(cams["cy"][i]),
                         int(cams["width"][i]), int(cams["height"][i]))


def _pop_unseen(unseen: List[int], count: int, rng: random.Random) -> int:
    """full_images_datamanager.py:305-308: a random index leaves the unseen list, which is refilled once it is empty."""
    idx = unseen.pop(rng.randint(0, len(unseen) - 1))
    if not unseen:
        unseen.extend(range(count))
    return idx


class ThermalFullImageDatamanager:
    def __init__(self, config: ThermalFullImageDatamanagerConfig, device="cuda"):
        self.config = config
        self.device = torch.device(device)
        self.dataparser = config.dataparser.setup()
        self.train_dataparser_outputs = self.dataparser.get_dataparser_outputs("train")
        self.eval_dataparser_outputs = self.dataparser.get_dataparser_outputs(config.eval_split)
        self.cached_train, self.train_cameras = self._cache(self.train_dataparser_outputs, train=True)
        self.cached_eval, self.eval_cameras = self._cache(self.eval_dataparser_outputs)
        if not self.cached_train:
            raise ValueError("No data found in dataset")
        self.rng = random.Random(config.seed)
        self.train_unseen_cameras = list(range(len(self.cached_train)))
        self.eval_unseen_cameras = list(range(len(self.cached_eval)))
        self._last_pixels = 0

    def _cache(self, outputs: DataparserOutputs, train: bool = False) -> Tuple[List[Batch], List[PinholeCamera]]:
        """Every camera carries its spectrum (is_thermal); a training camera also its index among the training frames (cam_idx), the row of a
        per-frame pose optimiser."""
        load = load_image_uint8 if self.config.cache_images_type == "uint8" else load_image_float32
        cached, cameras = [], []
        for i, path in enumerate(outputs.image_filenames):
            image, camera = load(path).to(self.device), parsed_camera(outputs, i)
            if self.config.undistort:
                image, camera = undistort_image(image, camera, outputs.cameras["distortion"][i])
            is_thermal = bool(outputs.metadata["is_thermal"][i])
            cached.append({"image": image, "is_thermal": is_thermal, "image_idx": i})
            cameras.append(dataclasses.replace(camera, cam_idx=i if train else None, is_thermal=is_thermal))
        return cached, cameras

    @property
    def num_train_data(self) -> int:
        return len(self.cached_train)

    @property
    def train_is_thermal(self) -> List[bool]:
        """One flag per training frame: what ThermalSplatfactoModel(train_is_thermal=...) marks the other spectrum's pose rows with."""
        return [bool(b["is_thermal"]) for b in self.cached_train]

    @property
    def seed_points(self) -> Optional[Tuple[Tensor, ...]]:
        """The dataparser's (points3D_xyz, points3D_rgb) (config.dataparser.load_3D_points), or None when the dataset has no cloud.  A cloud with
        thermal values (points3D_thermal: a PLY with the `thermal` property, as cloud.py exports it) comes as the 3-tuple (xyz, rgb, thermal)."""
        meta = self.train_dataparser_outputs.metadata
        if "points3D_xyz" not in meta:
            return None
        if "points3D_thermal" in meta:
            return meta["points3D_xyz"], meta["points3D_rgb"], meta["points3D_thermal"]
        return meta["points3D_xyz"], meta["points3D_rgb"]

    def _serve(self, cached: List[Batch], cameras: List[PinholeCamera], idx: int) -> Tuple[PinholeCamera, Batch]:
        batch = dict(cached[idx])
        self._last_pixels = int(batch["image"].shape[0] * batch["image"].shape[1])
        return cameras[idx], batch

    def next_train(self, step: int) -> Tuple[PinholeCamera, Batch]:
        """full_images_datamanager.py:301-318: a frame no step has seen since the list was last full, and its camera."""
        return self._serve(self.cached_train, self.train_cameras, _pop_unseen(self.train_unseen_cameras, len(self.cached_train), self.rng))

    def next_eval(self, step: int) -> Tuple[PinholeCamera, Batch]:
        """:320-332, over the eval split."""
        if not self.cached_eval:
            raise ValueError(f"the {self.config.eval_split!r} split is empty")
        return self._serve(self.cached_eval, self.eval_cameras, _pop_unseen(self.eval_unseen_cameras, len(self.cached_eval), self.rng))

    def next_eval_image(self, step: int) -> Tuple[PinholeCamera, Batch]:
        """:334-348: the reference draws it as next_eval does."""
        return self.next_eval(step)

    @property
    def fixed_indices_eval_dataloader(self) -> List[Tuple[PinholeCamera, Batch]]:
        """:275-288: every eval frame once, in the split's order."""
        return [(self.eval_cameras[i], dict(self.cached_eval[i])) for i in range(len(self.cached_eval))]

    def get_param_groups(self) -> Dict[str, list]:
        return {}

    def get_train_rays_per_batch(self) -> int:
        """The pixel count of the last frame served (the reference returns a placeholder, :297-299)."""
        return self._last_pixels
