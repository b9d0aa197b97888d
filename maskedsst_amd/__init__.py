"""maskedsst_amd -- MI355X-native (gfx950) implementation of the MaskedSST masked-pretraining hot path.

Drop-in mirrors of the reference modules (same constructor / attribute / state_dict surface):

    from maskedsst_amd import ViTSpatialSpectral, SimMIMSpatialSpectral

Compute runs in hand-written HIP kernels (``maskedsst_amd/csrc``) behind the C-ABI of
``include/msst.h`` (``libmsst.so``, loaded with ctypes).  There is no CPU or eager fallback.
"""
from .vit_spatial_spectral import ViTSpatialSpectral  # noqa: F401
from .vit_simmim_original import SimMIMSpatialSpectral, BlockwiseToPixels, Reconstruction, SceneReconstruction  # noqa: F401
from .recon import recon_report, ReconReport, window_masks_to_scene, scene_mask_to_windows  # noqa: F401
from .masking import MaskGenerator, micro_masks, DeviceMasks  # noqa: F401
from .optim import GradAccumulator  # noqa: F401
from .scene import SceneEmbedding, centre_origins, random_origins, window_labels, orient_windows, random_orients  # noqa: F401
from .saliency import input_gradient, band_importance, integrated_gradients, scene_saliency, band_importance_scene, SceneSaliency  # noqa: F401
from .attention import AttentionMaps, attention_rollout, attention_received  # noqa: F401
from .knn import KnnBank, KnnResult, KnnScene, feature_bank, knn_classify, knn_predict_scene  # noqa: F401
from .probe import LinearProbe, ProbeScene, fit_linear_probe, probe_bank, probe_gradient, probe_predict_scene  # noqa: F401
from .cluster import KMeans, ClusterScene, ClusterMatch, fit_kmeans, cluster_scene, contingency, match_clusters  # noqa: F401
from .pca import FeaturePCA, PcaScene, AnomalyScene, fit_pca, pca_scene, anomaly_scene  # noqa: F401
from .gaussian import GaussianClassifier, GaussianResult, GaussianScene, fit_gaussian, gaussian_predict_scene  # noqa: F401
from .mixture import GaussianMixture, MixtureResult, MixtureScene, fit_mixture, mixture_scene  # noqa: F401
from .crf import CrfAffinity, CrfResult, RefinedScene, crf_affinity, crf_refine, refine_scene  # noqa: F401
from .superpixel import (Superpixels, ObjectResult, SuperpixelScene, SlicCentres, fit_superpixels, superpixel_pool,  # noqa: F401
                         superpixel_classify, superpixel_assign, superpixel_update, superpixel_scene)
from .regions import (Regions, SieveResult, ConnectedSuperpixels, label_regions, region_ids, check_regions, sieve_classes,  # noqa: F401
                      enforce_connectivity)

__all__ = ["ViTSpatialSpectral", "SimMIMSpatialSpectral", "BlockwiseToPixels", "MaskGenerator", "Reconstruction", "recon_report",
           "ReconReport", "SceneReconstruction", "window_masks_to_scene", "scene_mask_to_windows", "SceneEmbedding",
           "input_gradient", "band_importance", "integrated_gradients", "AttentionMaps", "attention_rollout", "attention_received",
           "centre_origins", "random_origins", "window_labels", "orient_windows", "random_orients", "scene_saliency", "band_importance_scene", "SceneSaliency",
           "GradAccumulator", "micro_masks", "DeviceMasks",
           "KnnBank", "KnnResult", "KnnScene", "feature_bank", "knn_classify", "knn_predict_scene",
           "LinearProbe", "ProbeScene", "fit_linear_probe", "probe_bank", "probe_gradient", "probe_predict_scene",
           "KMeans", "ClusterScene", "ClusterMatch", "fit_kmeans", "cluster_scene", "contingency", "match_clusters",
           "FeaturePCA", "PcaScene", "AnomalyScene", "fit_pca", "pca_scene", "anomaly_scene",
           "GaussianClassifier", "GaussianResult", "GaussianScene", "fit_gaussian", "gaussian_predict_scene",
           "GaussianMixture", "MixtureResult", "MixtureScene", "fit_mixture", "mixture_scene",
           "CrfAffinity", "CrfResult", "RefinedScene", "crf_affinity", "crf_refine", "refine_scene",
           "Superpixels", "ObjectResult", "SuperpixelScene", "SlicCentres", "fit_superpixels", "superpixel_pool", "superpixel_classify",
           "superpixel_assign", "superpixel_update", "superpixel_scene",
           "Regions", "SieveResult", "ConnectedSuperpixels", "label_regions", "region_ids", "check_regions", "sieve_classes",
           "enforce_connectivity"]
