"""The weights of LPIPS (lpips.LPIPS(net='alex'), version 0.1) for rnerf_lpips (csrc/lpips.hip): ops.lpips, utils.compute_lpips,
errmap.error_maps(lpips=...), evaluate.evaluate(lpips=...).

No weights are part of this repository and none are made up here: load_weights reads the two published files a user has
(torchvision's alexnet-owt-7be5be79.pth and lpips' weights/v0.1/alex.pth), or one file holding lpips.LPIPS(net='alex').state_dict();
from_tensors takes the fifteen tensors directly.  Both give a Weights object whose `flat` is the one float32 device buffer of
include/rnerf.h: conv1.weight, conv1.bias, ..., conv5.weight, conv5.bias, lin0 .. lin4, each in torch's own layout.  Parity with the
published weights is unpinned: the network is restated from the package's definition, and the files were not at hand to confirm one
end-to-end number."""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import torch

from ._lib import LPIPS_WEIGHT_FLOATS, RnerfError

# (Cout, Cin, k) of the five convolutions; the index of each in torchvision's alexnet.features and lpips' slice it sits in
CONV_SHAPES = ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))
FEATURE_INDEX = (0, 3, 6, 8, 10)
ALEXNET_KEYS = tuple(f"features.{i}" for i in FEATURE_INDEX)
STATE_DICT_KEYS = tuple(f"net.slice{s + 1}.{i}" for s, i in enumerate(FEATURE_INDEX))
LIN_KEYS = tuple(f"lin{l}.model.1.weight" for l in range(5))


@dataclasses.dataclass(frozen=True)
class Weights:
    """flat: float32 [LPIPS_WEIGHT_FLOATS] on the device, the layout of include/rnerf.h (rnerf_lpips)."""
    flat: torch.Tensor

    @property
    def device(self) -> torch.device:
        return self.flat.device


def _device(device) -> torch.device:
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _take(t, shape, key: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise RnerfError(f"lpips weights: {key} is not a tensor")
    if tuple(t.shape) != tuple(shape):
        raise RnerfError(f"lpips weights: {key} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.detach().to(dtype=torch.float32, device="cpu").reshape(-1)


def flatten(convs: Sequence, biases: Sequence, lins: Sequence, names=None) -> torch.Tensor:
    """The flat CPU buffer of rnerf_lpips from convs[l]: [Cout, Cin, k, k], biases[l]: [Cout], lins[l]: [1, C_l, 1, 1] (or [C_l])."""
    if len(convs) != 5 or len(biases) != 5 or len(lins) != 5:
        raise RnerfError(f"lpips weights: need 5 convolutions, 5 biases and 5 lin layers, got {len(convs)}, {len(biases)}, {len(lins)}")
    names = names or ([f"convs[{l}]" for l in range(5)], [f"biases[{l}]" for l in range(5)], [f"lins[{l}]" for l in range(5)])
    parts = []
    for l, (co, ci, k) in enumerate(CONV_SHAPES):
        parts.append(_take(convs[l], (co, ci, k, k), names[0][l]))
        parts.append(_take(biases[l], (co,), names[1][l]))
    for l, (co, _, _) in enumerate(CONV_SHAPES):
        t = lins[l]
        shape = (co,) if isinstance(t, torch.Tensor) and t.dim() == 1 else (1, co, 1, 1)
        parts.append(_take(t, shape, names[2][l]))
    flat = torch.cat(parts)
    assert flat.numel() == LPIPS_WEIGHT_FLOATS
    return flat


def from_tensors(convs: Sequence, biases: Sequence, lins: Sequence, device=None) -> Weights:
    """A weights object from the tensors themselves (any device, any float dtype); a mis-shaped tensor raises RnerfError naming it."""
    return Weights(flatten(convs, biases, lins).to(_device(device)))


def _load(path: str) -> dict:
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise RnerfError(f"lpips weights: {path} does not hold a state dict")
    return sd


def _pick(sd: dict, key: str, path: str):
    if key not in sd:
        raise RnerfError(f"lpips weights: {path} has no key {key}")
    return sd[key]


def flat_from_files(alexnet_path: Optional[str] = None, lin_path: Optional[str] = None, state_dict_path: Optional[str] = None) -> torch.Tensor:
    """The flat CPU buffer from the published files (see load_weights)."""
    if state_dict_path is not None:
        if alexnet_path is not None or lin_path is not None:
            raise ValueError("lpips.load_weights: give state_dict_path, or alexnet_path and lin_path, not both")
        conv_sd = lin_sd = _load(state_dict_path)
        conv_path = lin_path = state_dict_path
        prefixes = STATE_DICT_KEYS
    else:
        if alexnet_path is None or lin_path is None:
            raise ValueError("lpips.load_weights: need alexnet_path and lin_path (or state_dict_path)")
        conv_sd, lin_sd, conv_path, prefixes = _load(alexnet_path), _load(lin_path), alexnet_path, ALEXNET_KEYS
    w_names, b_names = [p + ".weight" for p in prefixes], [p + ".bias" for p in prefixes]
    convs = [_pick(conv_sd, k, conv_path) for k in w_names]
    biases = [_pick(conv_sd, k, conv_path) for k in b_names]
    lins = [_pick(lin_sd, k, lin_path) for k in LIN_KEYS]
    return flatten(convs, biases, lins, (w_names, b_names, list(LIN_KEYS)))


def load_weights(alexnet_path: Optional[str] = None, lin_path: Optional[str] = None, state_dict_path: Optional[str] = None,
                 device=None) -> Weights:
    """alexnet_path: torchvision's alexnet-owt-7be5be79.pth (keys features.{0,3,6,8,10}.{weight,bias}; classifier.* is ignored) and
    lin_path: lpips' weights/v0.1/alex.pth (keys lin{0..4}.model.1.weight, [1, C, 1, 1]); or state_dict_path: one file holding
    lpips.LPIPS(net='alex').state_dict() (keys net.slice1.0.*, net.slice2.3.*, net.slice3.6.*, net.slice4.8.*, net.slice5.10.*,
    lin{l}.model.1.weight).  Read with torch.load(..., weights_only=True); a missing or mis-shaped key raises RnerfError naming it."""
    return Weights(flat_from_files(alexnet_path, lin_path, state_dict_path).to(_device(device)))
