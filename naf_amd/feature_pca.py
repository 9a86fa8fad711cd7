"""Feature PCA for display: the reference's ``pca()`` / ``TorchPCA`` (utils/visualization.py:135-190) with the maps left on the device.

The fit needs each map's second moments (``ops.feature_moments``: Gram matrix and channel sums on the matrix cores) and a C x C
eigen-decomposition; a map's picture is its projection on the basis (``ops.pca_project``) scaled by the minima and maxima that call
returns.  With a fitted basis the projection is a linear head, so ``pca.normalize(naf(image, feats, size, head=pca.head()))`` is the
picture of an upsampled map that was never written.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import ops


def _eigh(S: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp64 eigen-decomposition of the C x C covariance: on the device where the installed torch can, on the host otherwise (not a hot path)."""
    try:
        return torch.linalg.eigh(S)
    except RuntimeError:
        w, v = torch.linalg.eigh(S.cpu())
        return w.to(S.device), v.to(S.device)


class FeaturePCA:
    """``FeaturePCA(n_components=3).fit(maps)``: principal components of feature maps for display.

    ``fit(maps)`` takes one map ``[1, C, H, W]`` / ``[C, H, W]`` or a list of maps with the same C (bf16 or fp32; see
    ``ops.feature_moments`` for what is copied).  Each map is weighted by ``1 / P_m`` (P_m = its pixel count), so every map counts the
    same: the mean is ``mu = (1/M) sum_m sum_m / P_m`` and the covariance ``S = (1/M) sum_m gram_m / P_m - mu mu^T``, formed in fp64.  This
    is the reference's fit whenever all maps have the first map's size and are square.  The reference otherwise resizes every map
    bilinearly to ``(H0, H0)`` of the first map before fitting (visualization.py:138-149); THIS FIT DOES NOT RESIZE, it weights.
    The basis is the top ``n_components`` eigenvectors of S (``torch.linalg.eigh`` in fp64) in descending order of eigenvalue; each
    eigenvector's sign is fixed so that its entry of largest magnitude is positive (the lowest index wins ties).  The reference's signs
    are whatever ``torch.pca_lowrank`` returns; these are defined.

    Attributes after ``fit`` (fp64, on the maps' device), mirroring ``TorchPCA``: ``mean_`` [C], ``components_`` [C, n],
    ``singular_values_`` [n] = sqrt(M P_0 eigenvalue) (P_0 the first map's pixel count: the singular values of the reference's stacked,
    centred matrix), and in addition ``explained_variance_`` [n], the eigenvalues.
    """

    def __init__(self, n_components: int = 3):
        if not isinstance(n_components, int) or isinstance(n_components, bool):
            raise TypeError(f"naf_amd.FeaturePCA: n_components must be an int, got {type(n_components).__name__}")
        if not 1 <= n_components <= 8:
            raise ValueError(f"naf_amd.FeaturePCA: n_components = {n_components}; served: 1 <= n_components <= 8")
        self.n_components = n_components
        self.mean_ = self.components_ = self.singular_values_ = self.explained_variance_ = None
        self._V32 = self._b32 = None

    # ---- fit ----
    def fit(self, maps: Union[torch.Tensor, Sequence[torch.Tensor]]) -> "FeaturePCA":
        who = "FeaturePCA.fit"
        if torch.is_tensor(maps):
            maps = [maps]
        maps = list(maps)
        if not maps:
            raise ValueError(f"naf_amd.{who}: no maps")
        shapes = [ops._pca_map_shape(m, who, f"maps[{i}]") for i, m in enumerate(maps)]     # every map checked before any device work
        C_ = shapes[0][0]
        for i, s in enumerate(shapes):
            if s[0] != C_:
                raise ValueError(f"naf_amd.{who}: maps[{i}] has C = {s[0]} channels, maps[0] has {C_}")
        if self.n_components > C_:
            raise ValueError(f"naf_amd.{who}: n_components = {self.n_components} exceeds C = {C_}")
        for i, m in enumerate(maps):
            ops._gpu(m, f"maps[{i}]")
        G = mu = None
        for m in maps:
            gram, total, P = ops.feature_moments(m)
            G = gram / P if G is None else G + gram / P
            mu = total / P if mu is None else mu + total / P
        M = len(maps)
        mu = mu / M
        S = G / M - torch.outer(mu, mu)
        w, v = _eigh(S)
        n = self.n_components
        lam = w.flip(0)[:n].contiguous()
        V = v.flip(1)[:, :n].contiguous()
        idx = V.abs().argmax(dim=0)                                     # the first maximum: the lowest index wins ties
        V = V * torch.where(V.gather(0, idx.unsqueeze(0)) < 0, -1.0, 1.0)
        self.mean_, self.components_, self.explained_variance_ = mu, V, lam
        self.singular_values_ = (lam.clamp_min(0.0) * (M * shapes[0][1] * shapes[0][2])).sqrt()
        self._V32 = V.float().contiguous()
        self._b32 = (-(mu @ V)).float().contiguous()                    # formed in fp64, rounded once
        return self

    def _fitted(self, who: str) -> None:
        if self.components_ is None:
            raise RuntimeError(f"naf_amd.FeaturePCA.{who}: call fit() first")

    # ---- use ----
    def head(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(weight [n, C] fp32 = components_^T, bias [n] fp32 = -mean_ . components_)``: exactly the pair
        ``naf(image, feats, size, head=...)`` accepts; its output is ``transform`` of the upsampled map, which is then never written."""
        self._fitted("head")
        return self._V32.t().contiguous(), self._b32

    def _project(self, map: torch.Tensor, who: str):
        self._fitted(who)
        C_ = ops._pca_map_shape(map, f"FeaturePCA.{who}")[0]
        if C_ != self._V32.shape[0]:
            raise ValueError(f"naf_amd.FeaturePCA.{who}: the map has C = {C_} channels, the fit has {self._V32.shape[0]}")
        return ops.pca_project(map, self._V32, self._b32)

    def transform(self, map: torch.Tensor) -> torch.Tensor:
        """The raw projection ``(x - mean_) . components_`` of one map: fp32 ``[1, n, H, W]`` (a channels-last view)."""
        return self._project(map, "transform")[0]

    def transform_rgb(self, map: torch.Tensor) -> torch.Tensor:
        """The projection min-max normalised per component to [0, 1], ``(y - min) / (max - min)`` as visualization.py:166-167 does (a
        constant component divides by zero there, and it does here): fp32 ``[1, n, H, W]``."""
        raw, mm = self._project(map, "transform_rgb")
        lo, hi = mm[0].view(1, -1, 1, 1), mm[1].view(1, -1, 1, 1)
        return (raw - lo) / (hi - lo)

    @staticmethod
    def normalize(raw: torch.Tensor) -> torch.Tensor:
        """The same normalisation of an existing fp32 projection ``[B, n, H, W]``, per image and component -- for projections that came
        out of the head kernel."""
        if not torch.is_tensor(raw) or raw.dim() != 4:
            raise ValueError("naf_amd.FeaturePCA.normalize: `raw` must be a [B, n, H, W] tensor")
        mm = ops.pca_minmax(raw)
        lo, hi = mm[:, 0, :, None, None], mm[:, 1, :, None, None]
        return (raw - lo) / (hi - lo)


def pca(image_feats_list: List[torch.Tensor], dim: int = 3, fit_pca: Optional[FeaturePCA] = None) -> Tuple[List[torch.Tensor], FeaturePCA]:
    """The reference's ``pca(image_feats_list, dim=3, fit_pca=None)`` (utils/visualization.py:135-171) on the device: returns
    ``(list of [1, dim, H, W] fp32 pictures in [0, 1], fit)``, so ``plot_feats`` ports by changing the import and dropping ``.cpu()``.
    Like the reference, every map has B = 1.  Unlike it, maps of unequal sizes are weighted, not resized (``FeaturePCA``), component
    signs are defined, and ``max_samples`` is not offered: sub-sampling existed to bound the host cost."""
    if torch.is_tensor(image_feats_list):
        raise TypeError("naf_amd.pca: `image_feats_list` must be a list of [1, C, H, W] maps")
    maps = list(image_feats_list)
    for i, m in enumerate(maps):
        if torch.is_tensor(m) and m.dim() != 4:
            raise ValueError(f"naf_amd.pca: image_feats_list[{i}] must be [1, C, H, W], got {tuple(m.shape)}")
    if fit_pca is None:
        fit_pca = FeaturePCA(n_components=dim).fit(maps)
    elif not isinstance(fit_pca, FeaturePCA):
        raise TypeError(f"naf_amd.pca: fit_pca must be a naf_amd.FeaturePCA, got {type(fit_pca).__name__}")
    return [fit_pca.transform_rgb(m) for m in maps], fit_pca
