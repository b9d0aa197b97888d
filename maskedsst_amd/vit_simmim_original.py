"""``SimMIMSpatialSpectral`` -- drop-in mirror of the reference masked-image-modelling wrapper.

Mirrors reference ``src/vit_simmim_original.py:139-340`` (constructor, attributes, ``state_dict``
keys ``mask_token`` / ``encoder.*`` / ``to_pixels.*``, ``forward(img) -> scalar loss``).  The
forward/backward arithmetic runs in the HIP kernels of ``libmsst.so``; mask generation stays on the
host by default and is bit-exact with the reference (``maskedsst_amd/masking.py``); ``mask_source = "device"`` draws the
masks in one HIP launch instead (``draw_masks_device``).
"""
import weakref
from collections import namedtuple

import numpy as np
import torch
from torch import nn

from .masking import MaskGenerator, topk_masks, inverse_csr
from .vit_spatial_spectral import ViTSpatialSpectral


# what SimMIMSpatialSpectral.reconstruct returns: cube [B, C, H, W] fp32, mask [B, C, H, W] bool (the token mask over the P bands of
# each token), band_err [B, C] float64 (sum of |prediction - input| over the band's masked pixels), band_cnt [B, C] int32 (how many)
Reconstruction = namedtuple("Reconstruction", ["cube", "mask", "band_err", "band_cnt"])
# what SimMIMSpatialSpectral.reconstruct_scene returns: the same four over a whole scene [Bs, C, Hs, Ws] -- mask: the scene mask over
# the P bands of each spectral block AND covered by a window (exactly the pixels band_cnt counts) -- and cover [Bs, Hs, Ws] int32, the
# number of windows covering a pixel
SceneReconstruction = namedtuple("SceneReconstruction", ["cube", "mask", "band_err", "band_cnt", "cover"])


class BlockwiseToPixels(nn.Module):
    """Parameter container for the per-spectral-block pixel decoders (reference :9-40);
    block id of a token = token index // num_spatial_patches."""

    def __init__(self, dim, num_spectral_blocks, pixels_per_patch, precision="32-true"):
        super().__init__()
        self.pixels_per_patch = pixels_per_patch
        self.layers = nn.ModuleList([nn.Linear(dim, pixels_per_patch) for _ in range(num_spectral_blocks)])
        if precision == "16-mixed":
            self.dtype = torch.float16
        elif precision == "32-true":
            self.dtype = torch.float32

    def forward(self, x, block_indices):
        raise RuntimeError("BlockwiseToPixels is fused into the masked-L1 head kernel (no eager fallback)")


class SimMIMSpatialSpectral(nn.Module):
    def __init__(self, *, encoder, masking_ratio=0.5, mask_patch_size=1, tube_masking=False,
                 intermediate_losses=False, to_pixels_per_spectral_block=False, precision="32-true"):
        super().__init__()
        assert masking_ratio > 0 and masking_ratio < 1, "masking ratio must be kept between 0 and 1"
        if not isinstance(encoder, ViTSpatialSpectral):
            raise NotImplementedError("only the ViTSpatialSpectral encoder is accelerated")
        if intermediate_losses:
            # the reference only supports this with the legacy _V1 encoder (it would NameError here)
            raise NotImplementedError("intermediate_losses requires the legacy ViTSpatialSpectral_V1 encoder")
        self.masking_ratio = masking_ratio
        self.mask_patch_size = mask_patch_size
        self.intermediate_losses = intermediate_losses
        self.to_pixels_per_spectral_block = to_pixels_per_spectral_block
        self.tube_masking = tube_masking
        if self.mask_patch_size != 1:
            self.mask_generator = MaskGenerator(
                input_size=encoder.image_size, mask_patch_size=mask_patch_size,
                model_patch_size=encoder.patch_height, mask_ratio=self.masking_ratio)
        self.encoder = encoder
        encoder_dim = encoder.dim
        self.to_patch = encoder.to_patch_embedding.to_patch
        self.patch_to_emb = encoder.to_patch_embedding.embed
        self.pixel_values_per_patch = encoder.pixels_per_patch
        self.mask_token = nn.Parameter(torch.randn(encoder_dim))
        if self.to_pixels_per_spectral_block:
            self.to_pixels = BlockwiseToPixels(encoder_dim, encoder.num_spectral_patches,
                                               self.pixel_values_per_patch, precision=precision)
        else:
            self.to_pixels = nn.Linear(encoder_dim, self.pixel_values_per_patch)
        self._engine = None
        encoder._engine_owner = weakref.ref(self)
        # data-parallel placement of this process: masks are drawn for the GLOBAL batch
        self.dp_rank, self.dp_world = 0, 1
        self.last_masks = None

    def engine(self):
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine(self.encoder, self)
        return self._engine

    # ------------------------------------------------------------------
    def draw_masks(self, batch):
        """Host-side masks for ``batch`` local samples (reference :252-282).  Under data parallel
        the global batch's masks are drawn on every rank and the local rows are sliced."""
        enc = self.encoder
        T = enc.num_patches
        num_masked = int(self.masking_ratio * T)
        gb = batch * self.dp_world
        if self.mask_patch_size == 1:
            bm, idx = topk_masks(gb, T, num_masked)
        elif self.tube_masking:   # closed form: only the local rows are materialised (RNG still advances globally)
            lo = self.dp_rank * batch
            return self.mask_generator.get_batch_tube_masked(gb, enc.num_spectral_patches, num_masked,
                                                             rows=(lo, lo + batch))
        else:
            bm, idx = self.mask_generator.get_batch(gb, enc.num_spectral_patches, num_masked)
        lo = self.dp_rank * batch
        return bm[lo:lo + batch], idx[lo:lo + batch]

    # ------------------------------------------------------------------ device-side masks (msst_draw_masks)
    @property
    def mask_source(self):
        """where masks come from when a caller passes none: "host" (default; ``draw_masks``, bit-exact with the reference's numpy and
        torch RNG streams) or "device" (``draw_masks_device``: one HIP launch, no host RNG beyond a seed, no upload)"""
        return self.__dict__.get("_mask_source", "host")

    @mask_source.setter
    def mask_source(self, value):
        if value not in ("host", "device"):
            raise ValueError(f'mask_source must be "host" or "device", got {value!r}')
        self.__dict__["_mask_source"] = value

    def _mask_draw_args(self):
        """(mode, rand_size, scale, mask_count, K) of msst_draw_masks for this model (reference :252-282's three branches)"""
        from . import _lib
        K = int(self.masking_ratio * self.encoder.num_patches)
        if self.mask_patch_size == 1:
            return _lib.MASK_TOPK, 0, 0, 0, K
        g = self.mask_generator
        return (_lib.MASK_TUBE if self.tube_masking else _lib.MASK_BLOCK), g.rand_size, g.scale, g.mask_count, K

    def draw_masks_device(self, batch, seed=None, device=None):
        """``DeviceMasks`` for ``batch`` local samples, drawn on the device in one launch: the token mask, the gather indices and the
        gather's token-CSR, rows [dp_rank batch, (dp_rank + 1) batch) of the seed's stream (a stateless counter hash: a row has the
        same bits in any batch, on any rank; nothing of the other ranks' rows is generated).  seed: an integer in [0, 2^32); None
        draws a 31-bit one from torch's CPU generator, the way the dropout seed is drawn, so that identically seeded ranks agree and
        ``torch.manual_seed`` reproduces a run.  device: default the model's.  The masks are NOT those of the host generator (no
        device reproduces its mt19937 streams): same distribution, other bits; index rows list their tokens ascending.
        ValueError -- before a device is asked for -- for a batch below 1 and a seed outside [0, 2^32)."""
        from . import _lib
        from .masking import DeviceMasks
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError(f"batch must be a positive integer, got {batch!r}")
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 32):
            raise ValueError(f"seed must be an integer in [0, 2^32), got {seed!r}")
        enc = self.encoder
        S, N, T = enc.num_spectral_patches, enc.num_spatial_patches, enc.num_patches
        mode, rand_size, scale, mask_count, K = self._mask_draw_args()
        if K < 1:
            raise ValueError(f"masking_ratio {self.masking_ratio} masks no token of {T}")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        dev = torch.device(device) if device is not None else self.mask_token.device
        if dev.type != "cuda":
            raise RuntimeError("maskedsst_amd runs on an MI355X only (device masks asked for on %s); there is no CPU fallback" % dev)
        batch, row0 = int(batch), int(self.dp_rank) * int(batch)
        bm = torch.empty((batch, T), dtype=torch.bool, device=dev)
        idx = torch.empty((batch, K), dtype=torch.int32, device=dev)
        ptr = torch.empty((batch, T + 1), dtype=torch.int32, device=dev)
        pos = torch.empty((batch, K), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.load().msst_draw_masks(bm.data_ptr(), idx.data_ptr(), ptr.data_ptr(), pos.data_ptr(), int(seed), row0, batch,
                                                   S, N, K, mode, rand_size, scale, mask_count, st), "msst_draw_masks")
        return DeviceMasks(bm, idx, ptr, pos, int(seed), row0)

    def _draw(self, batch, device=None):
        """the masks of a call that was handed none: the configured source's"""
        return self.draw_masks_device(batch, device=device) if self.mask_source == "device" else self.draw_masks(batch)

    def _check_device_masks(self, dm, rows):
        from .masking import check_device_masks
        check_device_masks(dm, rows, self.encoder.num_patches, int(self.masking_ratio * self.encoder.num_patches))

    def forward(self, img, masks=None):
        """img [B, bands, H, W] -> scalar reconstruction loss (mean |pred - target| / num_masked).  masks: None draws them from
        ``mask_source``; or the (bool_mask, idx) host pair; or a ``DeviceMasks``, which reaches the kernels as it is."""
        from .masking import DeviceMasks
        eng = self.engine()
        if isinstance(masks, DeviceMasks):
            self._check_device_masks(masks, img.shape[0])
        if masks is None:
            masks = self._draw(img.shape[0], getattr(img, "device", None))
        self.last_masks = masks
        if isinstance(masks, DeviceMasks):
            return eng.simmim_loss(img, masks)
        return eng.simmim_loss(img, masks[0], masks[1])

    # one window per row of the masked-L1 head's grid (msst_head_at_fwd)
    MAX_WINDOWS_AT = 65535

    def forward_at(self, tiles, origins, masks=None, check=True, orient=None):
        """forward(the stacked windows of tiles at origins, masks) without the stacked copy: pre-training on windows read straight out
        of resident tiles -- several windows per tile, or windows at chosen positions (labelled or cloud-free pixels).  tiles
        [Bs, bands, Ht, Wt] fp32 on the device; origins an integer tensor [n, 3] on either device, row i = (tile index, y0, x0) of the
        top-left pixel of window i.  Windows may overlap, repeat and come in any order.  masks: None draws ``draw_masks(n)``; or the
        (bool_mask, idx) pair ``forward`` takes, one row per window; ``last_masks`` is set as ``forward`` sets it.  -> the scalar loss,
        bit for bit ``self(stacked windows, masks)``, and through ``backward`` the same parameter gradients, in training (dropout) and
        in eval() / under no_grad.
        check=True validates the table's values (one reduction and one read-back) and raises ValueError naming the first row outside
        the tiles; check=False skips that read-back: the kernels then trust the table.  Raises ValueError -- before a device is asked
        for -- for tiles of the wrong rank, dtype or band count or smaller than one window, a table of the wrong shape or dtype or
        with no row or with more than 65535 rows, and masks that are not [n, tokens] / [n, masked tokens]; NotImplementedError for
        tiles that require a gradient (a fold of the tokenizer's input gradient plus the target's: not built).
        orient (D4 augmentation): an integer tensor [n] on either device, codes 0 .. 7 (``maskedsst_amd.orient_windows``): window i is
        read in orientation orient[i], by the tokenizer and by the head's target gather alike; masks are in the coordinates of the
        oriented window.  Loss and gradients have the bits of ``self(orient_windows(stacked windows, orient), masks)``.  Checked with
        the origins (ValueError for a wrong shape, dtype or value); None: the un-oriented entry points."""
        from .scene import _check_origins
        enc = self.encoder
        _check_origins(enc, tiles, origins, check, orient)
        if tiles.dtype != torch.float32:
            raise ValueError(f"tiles must be a float32 tensor, got {tiles.dtype}")
        n = origins.shape[0]
        if n < 1 or n > self.MAX_WINDOWS_AT:
            raise ValueError(f"origins lists {n} windows: one call takes 1 to {self.MAX_WINDOWS_AT} (one row of the head's grid each)")
        from .masking import DeviceMasks
        if isinstance(masks, DeviceMasks):   # shapes and dtypes only: nothing is read back
            self._check_device_masks(masks, n)
        elif masks is not None:
            T, K = enc.num_patches, int(self.masking_ratio * enc.num_patches)
            pair = [np.asarray(m.cpu() if torch.is_tensor(m) else m) for m in masks] if isinstance(masks, (tuple, list)) else []
            if len(pair) != 2 or pair[0].dtype != np.bool_ or pair[0].shape != (n, T) or pair[1].dtype.kind not in "iu" or pair[1].shape != (n, K):
                raise ValueError(f"masks must be the pair (bool [{n}, {T}] token mask, integer [{n}, {K}] masked token indices) that "
                                 f"draw_masks({n}) gives, got {[(str(m.dtype), m.shape) for m in pair] or type(masks)}")
        if tiles.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("forward_at gives no gradient for the tiles: it would be a fold of the tokenizer's input gradient "
                                      "plus the reconstruction target's over overlapping windows -- detach the tiles (parameter "
                                      "gradients are computed)")
        eng = self.engine()
        eng._require_cuda(tiles)
        if masks is None:
            masks = self._draw(n, tiles.device)
        self.last_masks = masks
        table = origins.to(device=tiles.device, dtype=torch.int32).contiguous()
        from .engine import Windows
        if orient is not None:
            orient = orient.to(device=tiles.device, dtype=torch.uint8).contiguous()
        src = Windows("listed", tiles, table, orient=orient)
        return eng.simmim_loss(src, masks) if isinstance(masks, DeviceMasks) else eng.simmim_loss(src, masks[0], masks[1])

    def forward_windows(self, tiles, masks=None):
        """forward(stack_image_batch(tiles), masks) without the stacked copy: the loss over every non-overlapping image_size x
        image_size window of tiles [B, bands, Ht, Wt], windows ordered (tile, window row, window column), trailing Ht % image_size rows
        and Wt % image_size columns dropped.  ``forward_at`` with that grid as its table: the same kernels, masks, errors and bits."""
        from .scene import scene_windows
        s = self.encoder.num_spatial_patches_sqrt
        if not torch.is_tensor(tiles) or tiles.dim() != 4:
            raise ValueError(f"scene must be a 4-D tensor [scenes, bands, H, W], got {getattr(tiles, 'shape', type(tiles))}")
        if tiles.shape[2] < s or tiles.shape[3] < s:
            raise ValueError(f"scene {tuple(tiles.shape)} is smaller than one {s} x {s} window")
        grid = scene_windows(tiles.shape[2], tiles.shape[3], s, s)
        table = torch.tensor([(b, y, x) for b in range(tiles.shape[0]) for y, x in grid], dtype=torch.int32).reshape(-1, 3)
        return self.forward_at(tiles, table, masks, check=False)

    def _token_mask(self, masks, B):
        """the bool [B, T] token mask of `masks`: the (bool_mask, idx) pair forward takes, or the bool mask alone"""
        T = self.encoder.num_patches
        bm = masks[0] if isinstance(masks, (tuple, list)) else masks   # (a DeviceMasks is a tuple: field 0 is the mask)
        bm = bm if torch.is_tensor(bm) else torch.from_numpy(np.asarray(bm))
        if bm.dtype != torch.bool or tuple(bm.shape) != (B, T):
            raise ValueError(f"mask must be a bool [{B}, {T}] tensor (batch, tokens), got {bm.dtype} {tuple(bm.shape)}")
        return bm

    @staticmethod
    def _mask_u8(bm, device):
        """the contiguous uint8 view the kernels read of a bool token mask: a bool mask already on the device is reinterpreted where
        it lies (a kernel-written DeviceMasks: no copy), anything else is converted and moved"""
        if bm.device == torch.device(device) and bm.is_contiguous():
            return bm.view(torch.uint8)
        return bm.to(device=device, dtype=torch.uint8).contiguous()

    def reconstruct(self, img, masks=None, blend=True):
        """What the model reconstructs: img [B, bands, H, W] -> Reconstruction(cube, mask, band_err, band_cnt).

        The tokens of `masks` are replaced by the mask token, the encoder runs as in ``forward`` in eval mode and ``to_pixels``
        is applied to EVERY token (one HIP pass, ``msst_recon_fwd``): ``cube`` holds the predicted pixels, with ``blend`` (default) the
        input's own pixels where nothing was masked -- the filled-in cube.  ``band_err / band_cnt`` is the mean absolute error of a
        band over its masked pixels, whatever ``blend`` is (``maskedsst_amd.recon_report`` sums it up).
        masks: None draws them as ``forward`` does (and sets ``last_masks``); or the (bool_mask, idx) pair ``forward`` takes; or a bare
        bool [B, T] tensor.  Always an eval forward under no_grad (no dropout), whatever the module's mode, which is left as it is."""
        enc = self.encoder
        s = enc.num_spatial_patches_sqrt
        C = enc.num_spectral_patches * enc.patch_depth
        if not torch.is_tensor(img) or img.dim() != 4:
            raise ValueError(f"img must be a 4-D tensor [batch, bands, H, W], got {getattr(img, 'shape', type(img))}")
        if img.shape[0] < 1 or tuple(img.shape[1:]) != (C, s, s):
            raise ValueError(f"img {tuple(img.shape)} is not [batch, {C}, {s}, {s}] (the model's bands and image size)")
        B = img.shape[0]
        if masks is None:
            masks = self._draw(B, img.device)
            self.last_masks = masks
        bm = self._token_mask(masks, B)
        eng = self.engine()
        eng._require_cuda(img)
        S, N, P = enc.num_spectral_patches, enc.num_spatial_patches, enc.pixels_per_patch
        mask_u8 = self._mask_u8(bm, img.device)
        recon, err, cnt = eng.reconstruct(img, mask_u8, blend)   # passes no dropout and saves nothing, whatever self.training
        mask = mask_u8.bool().view(B, S, 1, s, s).expand(B, S, P, s, s).reshape(B, C, s, s)
        return Reconstruction(recon.view(B, C, s, s), mask, err, cnt)

    def reconstruct_scene(self, scene, mask=None, stride=None, blend=True, max_windows=None):
        """``reconstruct`` for whole scenes: scene [Bs, bands, Hs, Ws] (any Hs, Ws >= image_size) with a mask in scene coordinates ->
        SceneReconstruction(cube, mask, band_err, band_cnt, cover).

        Every ``image_size`` window with origin 0, stride, 2 stride, ... is read straight out of the scene (tokens under the mask
        replaced by the mask token), all windows run as one batch (in chunks of ``max_windows``), and the per-window predictions are
        assembled on the device; overlapping windows (``stride < image_size``) are averaged.  With ``blend`` (default) every element
        whose token is not masked, and every pixel no window covers, is the input's own; without it covered pixels hold the
        prediction and uncovered pixels NaN.  ``band_err / band_cnt`` is the mean absolute error of a band over its masked, covered
        pixels (``maskedsst_amd.recon_report`` sums it up); ``cover`` the number of windows covering a pixel.
        mask: a bool [Bs, S, Hs, Ws] tensor (S spectral blocks; any device): dead detector columns, invalid bands, clouds.  None draws
        window masks as ``reconstruct`` does for Bs nr nq windows (sets ``last_masks``) and places them in scene coordinates
        (``maskedsst_amd.window_masks_to_scene``); that needs ``stride == image_size``, the default stride.
        Always an eval forward under no_grad (no dropout), whatever the module's mode, which is left as it is."""
        from .recon import window_masks_to_scene
        from .scene import _check_scene, SCENE_MAX_WINDOWS
        enc = self.encoder
        stride, max_windows = _check_scene(enc, scene, stride, SCENE_MAX_WINDOWS if max_windows is None else max_windows)
        Bs, C, Hs, Ws = scene.shape
        S, P, w = enc.num_spectral_patches, enc.pixels_per_patch, enc.num_spatial_patches_sqrt
        if mask is None:
            if stride != w:
                raise ValueError(f"mask=None draws one random mask per window, which needs non-overlapping windows: stride must be "
                                 f"{w} (the window size), got {stride}")
            nr, nq = (Hs - w) // w + 1, (Ws - w) // w + 1
            masks = self._draw(Bs * nr * nq, scene.device)
            self.last_masks = masks
            mask = window_masks_to_scene(self._token_mask(masks, Bs * nr * nq), Bs, S, Hs, Ws, w)
        elif not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (Bs, S, Hs, Ws):
            raise ValueError(f"mask must be a bool [{Bs}, {S}, {Hs}, {Ws}] tensor (scenes, spectral blocks, H, W), got "
                             f"{getattr(mask, 'dtype', type(mask))} {tuple(getattr(mask, 'shape', ()))}")
        eng = self.engine()
        eng._require_cuda(scene)
        mask_u8 = mask.to(device=scene.device, dtype=torch.uint8).contiguous()
        cube, err, cnt, cover = eng.reconstruct_scene(scene, mask_u8, stride, blend, max_windows)
        counted = (mask_u8.bool() & (cover > 0)[:, None]).view(Bs, S, 1, Hs, Ws).expand(Bs, S, P, Hs, Ws).reshape(Bs, C, Hs, Ws)
        return SceneReconstruction(cube, counted, err, cnt, cover)

    def attention_maps(self, img, masks=None, stack="both", reduce="mean", blocks=None):
        """``ViTSpatialSpectral.attention_maps`` of the encoder as the SimMIM model runs it: the tokens of `masks` are replaced by the
        mask token before the blocks.  masks: the (bool_mask, idx) pair ``forward`` takes or a bare bool [B, T] tensor; None = no
        token masked (the bare encoder's maps, bit for bit).  stack, reduce, blocks, the result, the precision rule and the errors:
        as there.  Always an eval forward under no_grad, whatever the module's mode, which is left as it is."""
        from .attention import _attention_maps
        mask_u8 = None
        if masks is not None:
            if not torch.is_tensor(img) or img.dim() != 4:
                raise ValueError(f"img must be a 4-D tensor [batch, bands, H, W], got {getattr(img, 'shape', type(img))}")
            mask_u8 = self._mask_u8(self._token_mask(masks, img.shape[0]), img.device)
        return _attention_maps(self.encoder, img, mask_u8, stack, reduce, blocks)
