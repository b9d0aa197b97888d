"""``ViTSpatialSpectral`` -- drop-in mirror of the reference encoder's ``nn.Module`` surface.

Mirrors reference ``src/vit_spatial_spectral.py:256-564`` (constructor signature, attributes read
across the SimMIM seam, ``state_dict`` key schema, parameter draw order -- SURVEY.md 8b / 3.4).
The modules below are *parameter containers*: the compute of the accelerated configuration
(blockwise patch embedding, spatial -> spectral factorised attention) runs in hand-written HIP
kernels through ``libmsst.so``; there is no eager / CPU fallback and calling a container's
``forward`` raises.
"""
from functools import reduce
from operator import mul

import numpy as np
import torch
from torch import nn

from .pos_embed import get_1d_sincos_pos_embed_from_grid, get_2d_sincos_pos_embed


def pair(t):
    return t if isinstance(t, tuple) else (t, t)


class _HipOnly(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError(
            f"{type(self).__name__} is a parameter container of the fused MI355X path; "
            "call ViTSpatialSpectral / SimMIMSpatialSpectral instead (no eager fallback).")


class PreNorm(_HipOnly):
    """reference :22-29"""

    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class FeedForward(_HipOnly):
    """reference :32-44 (Linear, GELU(erf), Dropout, Linear, Dropout)"""

    def __init__(self, dim, hidden_dim, dropout=0.0):
        super().__init__()
        self.net = nn.Sequential(
            nn.Linear(dim, hidden_dim), nn.GELU(), nn.Dropout(dropout),
            nn.Linear(hidden_dim, dim), nn.Dropout(dropout),
        )


class Attention(_HipOnly):
    """reference :47-78"""

    def __init__(self, dim, heads=8, dim_head=64, dropout=0.0):
        super().__init__()
        inner_dim = dim_head * heads
        project_out = not (heads == 1 and dim_head == dim)
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.attend = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.to_out = (nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))
                       if project_out else nn.Identity())


class Transformer(_HipOnly):
    """reference :81-104"""

    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout=0.0):
        super().__init__()
        self.layers = nn.ModuleList([])
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout)),
                PreNorm(dim, FeedForward(dim, mlp_dim, dropout=dropout)),
            ]))


class _Rearrange(nn.Module):
    """Placeholder for the einops ``Rearrange`` layers of the reference Sequential (:410-431): keeps
    the child indices (``spatial_spectral_transformer.1`` / ``.3``) of the state_dict schema.  The
    regrouping itself is done by strided addressing inside the kernels (no copies)."""

    def __init__(self, pattern):
        super().__init__()
        self.pattern = pattern

    def extra_repr(self):
        return self.pattern


class ToPatch(nn.Module):
    """``Rearrange('b (c p0)(h p1)(w p2) -> b c (h w)(p0 p1 p2)')`` (reference :197-202); a cheap
    view/permute kept callable because SimMIM exposes it as ``self.to_patch``."""

    def __init__(self, p0, p1, p2):
        super().__init__()
        self.p0, self.p1, self.p2 = p0, p1, p2

    def forward(self, x):
        b, C, H, W = x.shape
        c, h, w = C // self.p0, H // self.p1, W // self.p2
        x = x.reshape(b, c, self.p0, h, self.p1, w, self.p2).permute(0, 1, 3, 5, 2, 4, 6)
        return x.reshape(b, c, h * w, self.p0 * self.p1 * self.p2)


class BlockwisePatchEmbedding(nn.Module):
    """reference :178-229"""

    def __init__(self, num_channels, transformer_dim, patch_depth, patch_height, patch_width):
        super().__init__()
        assert num_channels % patch_depth == 0, \
            f"Number of channels {num_channels=} not divisible by patch_depth {patch_depth=}"
        self.patch_depth = patch_depth
        self.patch_height = patch_height
        self.patch_width = patch_width
        self.transformer_dim = transformer_dim
        self.patch_dim = reduce(mul, [patch_depth, patch_height, patch_width])
        self.num_blocks = num_channels // patch_depth
        self.pre_norm = nn.LayerNorm(self.patch_dim)
        self.post_norm = nn.LayerNorm(self.transformer_dim)
        self.to_patch = ToPatch(patch_depth, patch_height, patch_width)
        self.blockwise_embed = nn.ModuleList(
            [nn.Linear(self.patch_dim, self.transformer_dim) for _ in range(self.num_blocks)])
        self._owner = None  # set by ViTSpatialSpectral: the fused tokenizer lives in its engine

    def embed(self, patches):
        """tokens = LN(stack_i Linear_i(LN(patches[:, i]))) -- runs the HIP tokenizer (without
        position / mask terms) on patches laid out [B, S, N, P]."""
        return self._owner()._embed_patches(patches)

    def forward(self, x):
        return self.embed(self.to_patch(x))


class MoveAxis(nn.Module):
    def __init__(self, axes):
        super().__init__()
        self.axes = axes

    def forward(self, x):
        return torch.moveaxis(x, *self.axes)


class _HeadRearrange(nn.Module):
    """'b h w (p1 p2 num_classes) -> b (h p1) (w p2) num_classes' (reference :485-491)"""

    def __init__(self, p1, p2, num_classes):
        super().__init__()
        self.p1, self.p2, self.nc = p1, p2, num_classes

    def forward(self, x):
        b, h, w, _ = x.shape
        x = x.reshape(b, h, w, self.p1, self.p2, self.nc).permute(0, 1, 3, 2, 4, 5)
        return x.reshape(b, h * self.p1, w * self.p2, self.nc)


class _PixRearrange(nn.Module):
    """'b (p1 p2 num_classes) -> b p1 p2 num_classes' of the pixelwise head (reference :472-477)"""

    def __init__(self, p1, p2, num_classes):
        super().__init__()
        self.p1, self.p2, self.nc = p1, p2, num_classes

    def forward(self, x):
        return x.reshape(x.shape[0], self.p1, self.p2, self.nc)


class _Squeeze(nn.Module):
    """reference Squeeze: x.squeeze() -- [B, nc, 1, 1] -> [B, nc], or [nc] for a single sample"""

    def forward(self, x):
        return x.squeeze()


class ViTSpatialSpectral(nn.Module):
    """Same keyword-only constructor as reference :257-301.  Extra keyword ``precision``
    ('bf16' | 'fp32') selects the MFMA operand type of the fused kernels."""

    def __init__(self, *, image_size, spatial_patch_size, spectral_patch_size, num_classes, dim, depth,
                 heads, mlp_dim, spectral_pos_embed=True, pool="mean", blockwise_patch_embed=True,
                 channels=3, dim_head=64, dropout=0.0, emb_dropout=0.0,
                 spectral_pos=list(range(20)), spectral_only=False, spectral_mlp_head=False,
                 pixelwise=False, pos_embed_len=None, precision=None):
        super().__init__()
        image_height, image_width = pair(image_size)
        image_depth = channels
        self.patch_height, self.patch_width = pair(spatial_patch_size)
        self.patch_depth = spectral_patch_size
        self.image_size = image_size
        self.pixels_per_patch = reduce(mul, [self.patch_depth, self.patch_height, self.patch_width])
        self.spectral_pos = np.asarray(spectral_pos.tolist() if torch.is_tensor(spectral_pos) else spectral_pos)
        self.spectral_pos_embed = spectral_pos_embed
        self.blockwise_patch_embed = blockwise_patch_embed
        self.spectral_only = spectral_only
        self.spectral_mlp_head = spectral_mlp_head
        self.pixelwise = pixelwise
        assert (image_height % self.patch_height == 0 and image_width % self.patch_width == 0
                and image_depth % self.patch_depth == 0), \
            "Image dimensions must be divisible by the patch size."
        self.num_spatial_patches_sqrt = image_height // self.patch_height
        self.num_spatial_patches = self.num_spatial_patches_sqrt ** 2
        self.num_spectral_patches = image_depth // self.patch_depth
        self.num_patches = self.num_spatial_patches * self.num_spectral_patches
        assert pool in {"mean"}, "pool type must be either cls (cls token) or mean (mean pooling)"

        # ---- what the fused HIP path covers; everything else fails loudly (no eager fallback) ----
        unsupported = []
        if not blockwise_patch_embed:
            unsupported.append("blockwise_patch_embed=False")
        if spectral_only:
            unsupported.append("spectral_only=True")
        if pixelwise and spectral_mlp_head:
            unsupported.append("pixelwise=True with spectral_mlp_head=True")
        elif pixelwise and (image_height != image_width or image_height % 2 == 0):
            unsupported.append(f"pixelwise=True with image_size={image_size} (no centre pixel exists: the reference builds "
                               "pixelwise models at odd sizes, image_size - patch_sub)")
        elif pixelwise and num_classes > 32:
            unsupported.append(f"pixelwise=True with num_classes={num_classes} (the pixelwise head is built for <= 32)")
        if spectral_mlp_head and num_classes > 32:
            unsupported.append(f"spectral_mlp_head=True with num_classes={num_classes} (the spectral head is built for <= 32)")
        if dim != 96 or dim_head != 64 or mlp_dim != 64:
            unsupported.append(f"dim/dim_head/mlp_dim={dim}/{dim_head}/{mlp_dim} (kernels are built for 96/64/64)")
        if self.patch_height != 1 or self.patch_width != 1:
            unsupported.append("spatial_patch_size != 1")
        if self.num_spatial_patches > 64 or self.num_spectral_patches > 64 or self.patch_depth > 16:
            unsupported.append("more than 64 spatial / spectral tokens per sequence or spectral patch > 16")
        if unsupported:
            raise NotImplementedError(
                "maskedsst_amd accelerates the shipped MaskedSST configuration only; unsupported: "
                + ", ".join(unsupported))
        self.dropout_p = float(dropout)
        self.emb_dropout_p = float(emb_dropout)
        self.heads = heads
        self.depth = depth
        self.precision = precision

        self.to_patch_embedding = BlockwisePatchEmbedding(
            channels, dim, self.patch_depth, self.patch_height, self.patch_width)

        if self.spectral_pos_embed:
            channel_embed_dim = dim // 3
            pos_embed_dim = dim - channel_embed_dim
            self.pos_embed = nn.Parameter(torch.zeros(1, self.num_spatial_patches, pos_embed_dim))
            p_embed = get_2d_sincos_pos_embed(pos_embed_dim, self.num_spatial_patches_sqrt, cls_token=False)
            self.pos_embed.data.copy_(torch.from_numpy(p_embed).float().unsqueeze(0))
            assert len(self.spectral_pos) == self.num_spectral_patches, \
                f"{self.spectral_pos.shape=}, {self.num_spectral_patches=}"
            self.channel_embed = nn.Parameter(torch.zeros(1, self.num_spectral_patches, channel_embed_dim))
            chan_embed = get_1d_sincos_pos_embed_from_grid(channel_embed_dim, self.spectral_pos)
            self.channel_embed.data.copy_(torch.from_numpy(chan_embed).float().unsqueeze(0))
        else:
            if pos_embed_len is not None:
                self.pos_embedding = nn.Parameter(torch.randn(1, pos_embed_len, dim))
            else:
                self.pos_embedding = nn.Parameter(torch.randn(1, self.num_patches + 1, dim))

        self.dropout = nn.Dropout(emb_dropout)

        c, hw = self.num_spectral_patches, self.num_spatial_patches_sqrt
        self.spatial_spectral_transformer = nn.Sequential(
            _Rearrange("b (c h w) d -> (b c) (h w) d"),
            Transformer(dim, depth, heads, dim_head, mlp_dim, dropout),
            _Rearrange("(b c) (h w) d -> (b h w) c d"),
            Transformer(dim, depth, heads, dim_head, mlp_dim, dropout),
            _Rearrange("(b h w) c d -> b (c h w) d"),
        )
        self.pool = pool
        self.to_latent = nn.Identity()
        self.dim = dim
        num_out_pixels = self.patch_width * self.patch_height
        # spectral_mlp_head (reference :440-453): the S tokens of a position concatenated (96 S features) instead of averaged
        head_dim = dim * self.num_spectral_patches if spectral_mlp_head else dim
        if pixelwise:
            # centre-pixel classifier (reference :466-478): per-position LN(96), flatten [h, w, d] (feature n 96 + d,
            # n = h W + w), one Linear(96 N -> num_classes) per window, squeezed to [B, num_classes]
            self.mlp_head = nn.Sequential(
                nn.LayerNorm(dim),
                nn.Flatten(start_dim=1, end_dim=-1),
                nn.Linear(dim * self.num_spatial_patches, num_classes),
                _PixRearrange(self.patch_height, self.patch_width, num_classes),
                MoveAxis((-1, 1)),
                _Squeeze(),
            )
        else:
            self.mlp_head = nn.Sequential(
                nn.LayerNorm(head_dim),
                nn.Linear(head_dim, num_classes * num_out_pixels),
                _HeadRearrange(self.patch_height, self.patch_width, num_classes),
                MoveAxis((-1, 1)),
            )
        self.num_classes = num_classes

        import weakref
        self.to_patch_embedding._owner = weakref.ref(self)
        self._engine = None
        self._engine_owner = None  # a SimMIM wrapper installs its own engine (covers mask token + to_pixels)

    # ------------------------------------------------------------------
    def engine(self):
        if self._engine_owner is not None and self._engine_owner() is not None:
            return self._engine_owner().engine()
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine(self, None)
        return self._engine

    def get_pos_embeddings(self):
        """reference :501-516 -- [1, T, D] table (used for inspection; the kernels read the two
        factor tables directly)."""
        channel_embed = self.channel_embed.unsqueeze(2)
        pos_embed = self.pos_embed.unsqueeze(1)
        channel_embed = channel_embed.expand(-1, -1, pos_embed.shape[2], -1)
        pos_embed = pos_embed.expand(-1, channel_embed.shape[1], -1, -1)
        pos_channel = torch.cat((pos_embed, channel_embed), dim=-1)
        return pos_channel.reshape(1, self.num_patches, self.dim)

    def _embed_patches(self, patches):
        return self.engine().embed_patches(patches)

    def transformer_forward(self, x):
        """reference :495-499 -- both transformer stacks on tokens [B, T, D] (fused HIP blocks)."""
        return self.engine().transformer(x)

    def forward_features(self, img):
        """reference :518-534: tokenize + position + (emb dropout) + transformer."""
        return self.engine().features(img)

    def forward(self, img):
        """reference :536-564: features -> mean over the spectral axis (spectral_mlp_head: the S tokens of a position
        concatenated instead) -> LN -> Linear -> [B, num_classes, H, W].  pixelwise: mean over the spectral axis -> LN per
        position -> flatten -> Linear -> [B, num_classes] for the centre pixel ([num_classes] when B = 1: the reference's
        squeeze)."""
        return self.engine().classify(img)

    def forward_windows(self, tiles):
        """forward(stack_image_batch(tiles)) without the stacked copy (the reference's shifting_window training batch, src/utils.py
        :608-613, :451-474): logits of every non-overlapping image_size x image_size window of tiles [B, channels, Ht, Wt], windows
        ordered (tile, window row, window column), trailing Ht % image_size rows and Wt % image_size columns dropped ->
        [B nr nq, num_classes, image_size, image_size]; pixelwise: [B nr nq, num_classes].  Differentiable exactly as forward is, the
        same bits.  Raises ValueError for tiles of the wrong rank or band count, or smaller than one window; NotImplementedError in
        training mode with embedding dropout for more than 65535 windows per call of a model whose windows are not 8 x 8 with
        10-band patches (Engine.classify_tiles)."""
        s = self.num_spatial_patches_sqrt
        if tiles.dim() != 4:
            raise ValueError(f"tiles must be [B, channels, Ht, Wt], got {tuple(tiles.shape)}")
        bands = self.num_spectral_patches * self.patch_depth
        if tiles.shape[1] != bands:
            raise ValueError(f"tiles have {tiles.shape[1]} bands, the model expects {bands}")
        if tiles.shape[2] < s or tiles.shape[3] < s:
            raise ValueError(f"tiles of {tuple(tiles.shape[2:])} are smaller than one {s} x {s} window")
        return self.engine().classify_tiles(tiles)

    def forward_at(self, scene, origins, check=True, scene_grad=False, orient=None):
        """forward(the stacked windows of scene at origins) without the stacked copy: the sampling of a sparsely labelled scene (the
        reference's Houston2018Dataset, src/data_houston2018.py:303-329 -- a window centred at every labelled pixel, or windows at
        random positions).  scene [Bs, channels, Hs, Ws] fp32 on the device; origins an integer tensor [n, 3] on either device, row i
        = (scene index, y0, x0) of the top-left pixel of window i (maskedsst_amd.centre_origins / random_origins build such tables).
        Windows may overlap, repeat and come in any order.  -> [n, num_classes, image_size, image_size]; pixelwise: [n, num_classes]
        (forward's squeeze for n = 1).  Differentiable in the parameters exactly as forward is -- the same bits, in training (dropout,
        full finetune, linear_eval) and in eval().
        check=True validates the table's values (one reduction and one read-back) and raises ValueError naming the first row outside
        0 <= scene < Bs, 0 <= y0 <= Hs - image_size, 0 <= x0 <= Ws - image_size; check=False skips that read-back: the kernels then
        trust the table.  Raises ValueError -- before a device is asked for -- for a scene of the wrong rank or band count or smaller
        than one window, and for a table of the wrong shape or dtype or with no row; NotImplementedError for a scene that requires a
        gradient without scene_grad (the windows overlap: its gradient is an accumulating fold, opt-in), for an encoder wrapped in
        SimMIM under grad, and for the embedding-dropout limit of forward_windows.
        scene_grad=True: a scene that requires a gradient gets it -- scene.grad = the per-window input gradients (what forward gives
        the stacked windows) summed per pixel over the windows covering it, in the fixed order of msst_scene_fold_at (ascending y0, x0,
        row of the table): no atomics, equal bits on every run; zero where no window lies.  In training (dropout, full finetune,
        linear_eval) and on a frozen eval() model; the two launches only read, so the parameter gradients keep the bits of a run with
        the scene detached.
        orient (D4 augmentation): an integer tensor [n] on either device, one orientation code o = k + 4 f per window; window i is
        read as ``torch.rot90(torch.flip(w, (-1,)) if f else w, k, (-2, -1))`` of the window w at origins[i] -- where the kernels form
        its address: no oriented copy, no further launch.  The result and every parameter gradient have the bits of
        ``forward(maskedsst_amd.orient_windows(stacked windows, orient))``; the logits of a patch head are in the oriented frame
        (``orient_windows(logits, orient, inverse=True)`` maps them back, ``window_labels(..., orient=)`` gives their labels).  With
        check its range 0 .. 7 is verified in the origins' read-back; ValueError for a wrong shape, dtype or value;
        NotImplementedError together with scene_grad or a scene that requires a gradient.  None: the un-oriented entry points."""
        from .scene import forward_at
        return forward_at(self, scene, origins, check, scene_grad, orient)

    def predict_at(self, scene, origins, return_logits=False, max_windows=None, orient=None, tta=None):
        """Classes at listed windows (the Houston test protocol: predictions only where a label exists): forward_at under no_grad as
        an eval() model, whatever the module's mode, which is left unchanged, in chunks of at most max_windows windows (None:
        maskedsst_amd.scene.SCENE_MAX_WINDOWS; the result does not depend on it).  Returns classes = argmax over the class axis ([n, image_size, image_size] int64;
        pixelwise [n]) and, with return_logits, also the logits ([n, num_classes, image_size, image_size]; pixelwise [n, num_classes],
        never squeezed).  The table's values are always checked.
        orient [n]: forward_at's, passed through chunk by chunk (patch-head logits stay in the oriented frame).  tta="d4": test-time
        augmentation -- every window runs in all eight orientations, the logits of a patch head are mapped back onto the window's
        pixels (``orient_windows(..., inverse=True)``; a pixelwise model's need no mapping: the centre of an odd window is a fixed
        point of every orientation) and summed in ascending code order, then divided by eight: a fixed order, equal bits on every run
        and for every max_windows.  ValueError for an unknown tta, or tta together with orient."""
        from .scene import predict_at, SCENE_MAX_WINDOWS
        return predict_at(self, scene, origins, return_logits, SCENE_MAX_WINDOWS if max_windows is None else max_windows, orient, tta)

    def predict_scene(self, scene, stride=None, return_logits=False, max_windows=None):
        """Classify whole scenes [Bs, channels, Hs, Ws] with sliding windows of image_size (the window loop of the reference's
        inference_example.ipynb, one batched pass): returns the class map [Bs, Hs, Ws] (int64; -1 where no window covers a
        pixel) and, with return_logits, also the logit map [Bs, num_classes, Hs, Ws] (mean over the windows covering a pixel).
        stride: window step, 1 .. image_size (None: image_size, non-overlapping tiles).  A pixelwise model classifies the
        centre pixel of each window instead (None: stride 1, the dense per-pixel map of DeepHyperX's test()); every pixel that is
        no window's centre, the border of width image_size // 2 included, gets class -1 and logit 0.  Eval forward (no dropout) under
        no_grad whatever the module's mode, which is left unchanged; windows run in chunks of at most max_windows
        (None: maskedsst_amd.scene.SCENE_MAX_WINDOWS).  Raises ValueError for a scene of the wrong shape."""
        from .scene import predict_scene, SCENE_MAX_WINDOWS
        return predict_scene(self, scene, stride, return_logits, SCENE_MAX_WINDOWS if max_windows is None else max_windows)

    def encode_scene(self, scene, stride=None, normalize=False, max_windows=None):
        """Per-pixel embedding maps of whole scenes [Bs, channels, Hs, Ws] (fp32, on the device): the encoder's representation for
        k-NN / SVM on frozen features, clustering, change detection, retrieval.  Sliding windows of image_size, numbered and chunked as
        for predict_scene; no head runs, so every head kind, a bare encoder and an encoder inside a SimMIMSpatialSpectral all work.
        Returns SceneEmbedding(features, cover):
          features [Bs, 96, Hs, Ws] fp32: a window's feature at a position is the mean over the spectral tokens of the encoder output
            there (what the default head normalises); a pixel's feature is the plain mean of that over the windows covering it.  A
            pixel no window covers is NaN in all 96 channels (the convention of reconstruct_scene without blend).
          cover [Bs, Hs, Ws] int32: how many windows cover the pixel.
        stride: window step, 1 .. image_size (None: image_size, also for a pixelwise model).  normalize=True divides every covered
        pixel's 96-vector by max(||f||_2, 1e-12) (torch.nn.functional.normalize) after the averaging.  Eval forward (no dropout, no mask
        token) under no_grad at the model's precision on the current stream, whatever the module's mode, which is left unchanged;
        windows run in chunks of at most max_windows (None: maskedsst_amd.scene.SCENE_MAX_WINDOWS).  Raises ValueError for a scene of
        the wrong rank or band count, one smaller than a window, or a stride outside its range; a CPU tensor raises as everywhere."""
        from .scene import encode_scene, SCENE_MAX_WINDOWS
        return encode_scene(self, scene, stride, normalize, SCENE_MAX_WINDOWS if max_windows is None else max_windows)

    def knn_predict_scene(self, scene, bank, k=20, temperature=0.07, stride=None, max_windows=None):
        """Classify every pixel of whole scenes [Bs, channels, Hs, Ws] by the weighted vote of its k nearest neighbours in a bank of
        labelled features (maskedsst_amd.KnnBank, e.g. from maskedsst_amd.feature_bank): encode_scene(normalize=True), then
        msst_knn_topk and msst_knn_vote on the returned map in place -- no permuted copy and no score matrix.  Returns
        KnnScene(classes, votes, cover):
          classes [Bs, Hs, Ws] int64, -1 where no window covers the pixel;
          votes [Bs, n_classes, Hs, Ws] fp32 (the layout of predict_scene's logits): the sum of exp((s_j - s_1) / temperature) over
            the neighbours of each class, s_1 the best similarity (temperature = 0: the neighbour counts); 0 where uncovered;
          cover [Bs, Hs, Ws] int32 as from encode_scene.
        Neighbours are ranked by similarity descending, ties by bank index ascending, so the maps have the same bits in every call.
        stride, max_windows: encode_scene's.  No head runs: a bare encoder and the encoder of a SimMIMSpatialSpectral work.  The
        module's mode is left unchanged.  ValueError, before any device work, for a bank that is no KnnBank, k outside [1, 64], a
        negative temperature or a scene encode_scene refuses."""
        from .knn import knn_predict_scene
        return knn_predict_scene(self, scene, bank, k, temperature, stride, max_windows)

    def probe_predict_scene(self, scene, probe, stride=None, max_windows=None):
        """Classify every pixel of whole scenes [Bs, channels, Hs, Ws] with a linear probe (maskedsst_amd.LinearProbe, e.g. from
        maskedsst_amd.fit_linear_probe): encode_scene(normalize=False), then msst_probe_fwd -- LayerNorm(96) -> Linear -- on the
        returned map in place, no permuted copy.  Returns ProbeScene(classes, logits, cover):
          classes [Bs, Hs, Ws] int64: the argmax, ties to the lowest class; -1 where no window covers the pixel;
          logits [Bs, n_classes, Hs, Ws] fp32 (the layout of predict_scene's logits); NaN where uncovered;
          cover [Bs, Hs, Ws] int32 as from encode_scene.
        With overlapping windows (stride < image_size) this differs from probe.load_into(model) followed by predict_scene: here the
        FEATURES of the windows covering a pixel are averaged before the LayerNorm; predict_scene runs the head per window and
        averages the LOGITS.  At the default non-overlapping stride the two agree up to rounding.
        stride, max_windows: encode_scene's.  No head of the model runs, so every head kind and a bare encoder work.  The module's
        mode is left unchanged.  ValueError, before any device work, for a probe that is no LinearProbe or a scene encode_scene
        refuses."""
        from .probe import probe_predict_scene
        return probe_predict_scene(self, scene, probe, stride, max_windows)

    def cluster_scene(self, scene, km, stride=None, max_windows=None):
        """Segment whole scenes [Bs, channels, Hs, Ws] without labels: every pixel goes to the nearest centroid of a k-means clustering
        (maskedsst_amd.KMeans, e.g. from maskedsst_amd.fit_kmeans on the features of other scenes): encode_scene(normalize = (km.metric ==
        "cosine")), then msst_kmeans_assign on the returned map in place, no permuted copy and no distance matrix.  Returns
        ClusterScene(classes, distance, cover):
          classes [Bs, Hs, Ws] int64: the cluster of the largest score, ties to the lowest index; -1 where no window covers the pixel;
          distance [Bs, Hs, Ws] fp32: 2 (1 - x . c) (cosine) or |x - c|^2 (euclidean) to that centroid; NaN where uncovered;
          cover [Bs, Hs, Ws] int32 as from encode_scene.
        The maps have the same bits in every call and equal km.assign on the permuted map.  stride, max_windows: encode_scene's.  No
        head runs: a bare encoder and the encoder of a SimMIMSpatialSpectral work.  The module's mode is left unchanged.  ValueError,
        before any device work, for a km that is no KMeans or a scene encode_scene refuses."""
        from .cluster import cluster_scene
        return cluster_scene(self, scene, km, stride, max_windows)

    def pca_scene(self, scene, pca, stride=None, whiten=False, max_windows=None):
        """The principal-component maps of whole scenes [Bs, channels, Hs, Ws] under a maskedsst_amd.FeaturePCA (e.g. from
        maskedsst_amd.fit_pca on the features of other scenes; the first three maps are the usual false-colour picture of an
        embedding): encode_scene(normalize=False), then msst_feat_project on the returned map in place, no permuted copy.  Returns
        PcaScene(components, cover):
          components [Bs, r, Hs, Ws] fp32: (x - mean) . component_j per pixel; whiten=True: divided by sqrt(lambda_j), the maps from
                     pca.rank on dropped; NaN where no window covers the pixel;
          cover [Bs, Hs, Ws] int32 as from encode_scene.
        The maps have the same bits in every call and equal pca.transform on the permuted map.  stride, max_windows: encode_scene's.
        No head runs; the module's mode is left unchanged.  ValueError, before any device work, for a pca that is no FeaturePCA or a
        scene encode_scene refuses."""
        from .pca import pca_scene
        return pca_scene(self, scene, pca, stride, whiten, max_windows)

    def anomaly_scene(self, scene, pca=None, stride=None, max_windows=None):
        """The RX anomaly score of whole scenes [Bs, channels, Hs, Ws] on the frozen features: per pixel the squared Mahalanobis
        distance to the mean of a maskedsst_amd.FeaturePCA under its covariance (pca.mahalanobis: one whitening projection and a row
        norm, msst_feat_project on the encode_scene map in place).  pca=None: fitted on the scenes' own covered pixels (global RX;
        maskedsst_amd.fit_pca on the map, uncovered pixels skipped).  Returns AnomalyScene(score, cover, pca): score [Bs, Hs, Ws] fp32,
        NaN where no window covers the pixel; cover as from encode_scene; pca the FeaturePCA used.  stride, max_windows:
        encode_scene's.  No head runs; the module's mode is left unchanged.  ValueError for a pca that is neither None nor a
        FeaturePCA, one that keeps fewer than its `rank` components, or a scene encode_scene refuses."""
        from .pca import anomaly_scene
        return anomaly_scene(self, scene, pca, stride, max_windows)

    def gaussian_predict_scene(self, scene, clf, stride=None, max_distance=None, max_windows=None):
        """The maximum-likelihood class map of whole scenes [Bs, channels, Hs, Ws] under a maskedsst_amd.GaussianClassifier (from
        maskedsst_amd.fit_gaussian on a bank of raw features): encode_scene(normalize=False), then ONE msst_gauss_score launch on the
        returned map in place, no permuted copy.  Returns GaussianScene(classes, scores, distance, cover):
          classes   [Bs, Hs, Ws] int64: the argmax of the log joint density score_c(x) = log prior_c - 0.5 (d2_c(x) + logdet_c) - 48
                    log(2 pi) under the total order (score descending, then class ascending); -1 where no window covers the pixel;
                    -2 where max_distance is given and the distance exceeds it (the pixel is none of the classes);
          scores    [Bs, nc, Hs, Ws] fp32, the layout of predict_scene's logits; NaN where uncovered;
          distance  [Bs, Hs, Ws] fp32: d2 = |A_c (x - mu_c)|^2 of the predicted class, the open-set score; NaN where uncovered;
          cover     as from encode_scene.
        The maps have the same bits in every call and equal clf.classify on the permuted map.  stride, max_windows: encode_scene's.
        No head runs; the module's mode is left unchanged.  ValueError, before any device work, for a clf that is no
        GaussianClassifier, a max_distance that is negative or no number, or a scene encode_scene refuses."""
        from .gaussian import gaussian_predict_scene
        return gaussian_predict_scene(self, scene, clf, stride, max_distance, max_windows)

    def mixture_scene(self, scene, gm, stride=None, probs=False, max_windows=None):
        """The soft segmentation and the density of whole scenes [Bs, channels, Hs, Ws] under a maskedsst_amd.GaussianMixture (e.g. from
        maskedsst_amd.fit_mixture on the raw features of other scenes): encode_scene(normalize=False), then msst_gauss_score and
        msst_gmm_posterior on the returned map in place, no permuted copy.  Returns MixtureScene(classes, log_likelihood, distance,
        probs, cover):
          classes         [Bs, Hs, Ws] int64: the component of the largest score log w_c + log N(x; mu_c, Sigma_c) under the total order
                          (score descending, then index ascending); -1 where no window covers the pixel;
          log_likelihood  [Bs, Hs, Ws] fp32: log p(x) under the mixture, whose negative is the cluster-based RX anomaly score; NaN
                          where uncovered;
          distance        [Bs, Hs, Ws] fp32: d2 = |A_c (x - mu_c)|^2 of the predicted component; NaN where uncovered;
          probs           probs=True: [Bs, K, Hs, Ws] fp32, the responsibilities in the layout of predict_scene's logits (a score map
                          for refine_scene and superpixel_classify); NaN where uncovered.  Otherwise None;
          cover           as from encode_scene.
        The maps have the same bits in every call and equal gm.predict on the permuted map.  stride, max_windows: encode_scene's.
        No head runs; the module's mode is left unchanged.  ValueError, before any device work, for a gm that is no GaussianMixture
        or a scene encode_scene refuses."""
        from .mixture import mixture_scene
        return mixture_scene(self, scene, gm, stride, probs, max_windows)

    def refine_scene(self, scene, scores, embedding=None, stride=None, iters=5, unary="logits", unary_scale=1.0, **affinity_kwargs):
        """The class map of whole scenes [Bs, channels, Hs, Ws] after a feature-guided CRF (mean field, Potts compatibility) over the
        score maps `scores` [Bs, nc, Hs, Ws] of any scene classifier -- predict_scene's logits, probe_predict_scene's logits,
        gaussian_predict_scene's scores (unary="logits") or knn_predict_scene's votes (unary="votes"): ONE msst_crf_affinity launch on
        the feature map in place, then iters + 1 msst_crf_step launches.  Returns RefinedScene(classes, probs, history, cover):
          classes   [Bs, Hs, Ws] int64: the argmax of the last probabilities under the total order (value descending, then class
                    ascending); -1 where the pixel is dead (uncovered, features not finite or zero, a NaN score, no score above -inf);
          probs     [Bs, nc, Hs, Ws] fp32; NaN where dead;
          history   [iters] int64 on the CPU: the live pixels whose class changed in each step;
          cover     as from encode_scene.
        embedding=None runs encode_scene(normalize=True) (stride: encode_scene's); pass the SceneEmbedding a *_predict_scene call was
        made from to avoid a second encoder pass -- a raw map and a normalised one both work, the kernel forms the norms.
        affinity_kwargs: radius, w_appearance, theta_feature, theta_position, w_smooth, theta_smooth of maskedsst_amd.crf_affinity; the
        defaults are API defaults, not tuned on data.  The message is not normalised: border pixels are smoothed less.  The maps have
        the same bits in every call and equal crf_refine on encode_scene's map.  No head runs; the module's mode is left unchanged.
        ValueError, before any device work, for wrong shapes, dtypes or ranges, or a scene encode_scene refuses."""
        from .crf import refine_scene
        return refine_scene(self, scene, scores, embedding, stride, iters, unary, unary_scale, **affinity_kwargs)

    def superpixel_scene(self, scene, scores=None, embedding=None, stride=None, step=8, compactness=0.2, iters=10):
        """SLIC superpixels of whole scenes [Bs, channels, Hs, Ws] from the encoder's feature map and, with the score maps `scores`
        [Bs, nc, Hs, Ws] of any scene classifier (predict_scene's logits, probe_predict_scene's logits, gaussian_predict_scene's
        scores, knn_predict_scene's votes), the object-based class map: the scores pooled per superpixel, every pixel given its
        superpixel's class.  Returns SuperpixelScene(superpixels, classes, region_scores, cover):
          superpixels    maskedsst_amd.fit_superpixels' result (labels, centroids, positions, counts, history, step, grid);
          classes        [Bs, Hs, Ws] int64, -1 where the pixel is dead (uncovered, features not finite); None without scores;
          region_scores  [Bs, n_sp, nc] fp32, NaN for a superpixel without pixels; None without scores;
          cover          as from encode_scene.
        embedding=None runs encode_scene(normalize=True) (stride: encode_scene's); pass the SceneEmbedding a *_predict_scene call was
        made from to avoid a second encoder pass.  step in {4, 8, 16}; step, compactness and iters are API defaults, not tuned on
        data.  No connectivity enforcement.  The maps have the same bits in every call and equal fit_superpixels and
        superpixel_classify on encode_scene's map.  No head runs; the module's mode is left unchanged.  ValueError, before any device
        work, for wrong shapes, dtypes or ranges, or a scene encode_scene refuses."""
        from .superpixel import superpixel_scene
        return superpixel_scene(self, scene, scores, embedding, stride, step, compactness, iters)

    def attention_maps(self, img, stack="both", reduce="mean", blocks=None):
        """The attention probabilities of the transformer blocks for img [B, channels, image_size, image_size] (fp32, on the device):
        AttentionMaps(spatial, spectral), fp32 on the device; the stack not asked for is None.
          stack   "spatial" | "spectral" | "both".  A spatial sequence is the N = image_size^2 positions of one spectral block (L = N,
                  S sequences per sample); a spectral sequence the S spectral blocks of one position (L = S, N sequences per sample).
          blocks  layer indices within a stack (None: all, in order); nblk = len(blocks).
          reduce  "mean": spatial [B, nblk, heads, N, N], spectral [B, nblk, heads, S, S] -- the mean over the sample's sequences,
                  added in sequence order in fp32 and divided once;  None: every sequence, spatial [B, nblk, S, heads, N, N], spectral
                  [B, nblk, N, heads, S, S] -- B S heads N^2 4 bytes per spatial block (EnMAP window, 8 heads: 2.6 MB per sample and
                  block), B N heads S^2 4 bytes per spectral block.
        Rows are queries, columns keys; every row sums to 1 (the reference's `attn` before dropout, vit_spatial_spectral.py:67-74).
        Precision: the maps are the fp32 softmax (``msst_attn_maps``: fp32 LayerNorm, projections and scores, whatever the model's
        precision) of the block inputs that the model's own forward produced.  For a bf16 model they therefore differ from the
        probabilities inside its block kernel by the half rounding of that kernel's operands -- not by more.
        Eval forward (no dropout, no mask token) under no_grad on the current stream, whatever the module's mode, which is left
        unchanged; no gradient flows.  Raises ValueError, before any launch, for an img of the wrong rank, band count or size, an
        unknown stack or reduce, or a block index out of range; a CPU tensor raises as everywhere (no CPU fallback).  When a block's
        maps are not a multiple of 4 floats (toy shapes; never with 8 heads) the result is a strided view."""
        from .attention import _attention_maps
        return _attention_maps(self, img, None, stack, reduce, blocks)
