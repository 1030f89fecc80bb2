"""fissure_segmentation_amd -- MI355X-native hot path of kaftanski/fissure-segmentation.

Host side mirrors the reference's module layout (models/, losses/, utils/, shapes/) so that
`train.py` / `train_pc_ae.py` / `model_trainer.py` find the same names, constructor arguments,
`forward` signatures and `state_dict` keys; the arithmetic runs in hand-written HIP kernels reached
through the C ABI of `libfsg_hip.so` (include/fsg_hip.h).  There is no CPU fallback: modules raise
if their input is not on a GPU or the library is missing.
"""
from . import _lib  # noqa: F401  (fails loudly when libfsg_hip.so is absent)
from . import functional  # noqa: F401
from . import augmentations  # noqa: F401

__version__ = "0.1.0"


def install_reference_aliases():
    """Register this package's modules under the reference's import names (`models.dgcnn`,
    `losses.chamfer_loss`, ...) so unmodified reference scripts pick them up.  See INTEGRATION.md."""
    import importlib
    import sys
    pairs = {
        "models.dgcnn": ".models.dgcnn", "models.dgcnn_opensrc": ".models.dgcnn_opensrc",
        "models.folding_net": ".models.folding_net", "models.point_net": ".models.point_net",
        "models.point_seg_net": ".models.point_seg_net", "models.modelio": ".models.modelio",
        "models.access_models": ".models.access_models",
        "models.pointtransformer.pointops": ".models.pointtransformer.pointops",
        "models.pointtransformer.seg_model": ".models.pointtransformer.seg_model",
        "losses.chamfer_loss": ".losses.chamfer_loss", "losses.nnu_loss": ".losses.nnu_loss",
        "losses.access_losses": ".losses.access_losses", "losses.mesh_loss": ".losses.mesh_loss",
        "losses.dgssm_loss": ".losses.dgssm_loss", "models.dg_ssm": ".models.dg_ssm",
        "shape_model": ".shape_model", "shape_model.ssm": ".shape_model.ssm", "metrics": ".metrics",
        "shape_model.point_cloud_registration": ".shape_model.point_cloud_registration",
        "shape_model.generate_corresponding_points": ".shape_model.generate_corresponding_points",
        "data_processing.foerstner": ".data_processing.foerstner", "data_processing.point_features": ".data_processing.point_features",
        "data_processing.keypoint_extraction": ".data_processing.keypoint_extraction",
        "data_processing.fissure_enhancement": ".data_processing.fissure_enhancement",
        "data_processing.random_walk": ".data_processing.random_walk", "data_processing.find_lobes": ".data_processing.find_lobes",
        "utils.image_utils": ".utils.image_utils", "utils.general_utils": ".utils.general_utils",
        "utils.image_ops": ".utils.image_ops", "utils.fissure_utils": ".utils.fissure_utils",
        "data_processing.surface_fitting": ".data_processing.surface_fitting",
        "data_processing.surface_fitting_optimization": ".data_processing.surface_fitting_optimization",
        "models.divroc": ".models.divroc", "models.dpsr_utils": ".models.dpsr_utils", "models.dpsr_net": ".models.dpsr_net",
        "models.seg_logits_to_mesh": ".models.seg_logits_to_mesh", "losses.dpsr_loss": ".losses.dpsr_loss",
        "models.seg_cnn": ".models.seg_cnn", "models.mobilenet": ".models.mobilenet", "models.aspp_3d": ".models.aspp_3d",
        "data_processing.process_lung_mask": ".data_processing.process_lung_mask",
        "dseg_ae_regularization": ".dseg_ae_regularization",
    }
    for ref_name, ours in pairs.items():
        sys.modules[ref_name] = importlib.import_module(ours, __name__)
    # the reference keeps `pointcloud_surface_fitting` and `poisson_reconstruction` in data_processing/surface_fitting.py, this
    # package in modules of their own: under the reference's name all are found (a module object that carries the names of the three)
    import types
    both = types.ModuleType("data_processing.surface_fitting", "fissure_segmentation_amd.data_processing.surface_fitting + "
                            "fissure_segmentation_amd.data_processing.pointcloud_surface_fitting + "
                            "fissure_segmentation_amd.data_processing.poisson_reconstruction")
    for ours in (".data_processing.poisson_reconstruction", ".data_processing.pointcloud_surface_fitting",
                 ".data_processing.surface_fitting"):
        both.__dict__.update({k: v for k, v in vars(importlib.import_module(ours, __name__)).items() if not k.startswith("_")})
    sys.modules["data_processing.surface_fitting"] = both
