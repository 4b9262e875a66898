"""MI355X-native sampling hot path of IVRL/NoiseDiff."""
__version__ = "0.1.0"

__all__ = ["GaussianDiffusion", "NoiseDiffNet", "UNet_PosEmbV2", "UNet_PosEmbV2_NoPosition", "UNet_PosEmbV2_CameraCond", "LSID",
           "TrainableNoiseDiffNet", "TrainableLSID", "pack_raw", "load_pair", "to_bayer", "RealBatchBuilder", "PoissonGaussianBatchBuilder",
           "DiffusionBatchBuilder", "GenerationBatchBuilder", "balanced_sample_list", "kld_edges", "get_histogram",
           "histogram_counts", "kl_div_forward", "kl_div_inverse", "kl_div_sym", "kl_div_3", "noise_kld", "patch_std_mean", "poisson_lambda_by_patch",
           "LevelMoments", "level_curve", "theil_sen", "get_poisson_lambda", "get_poisson_lambda_all_images", "get_regression_result_all_images",
           "Develop", "gamma_curve", "postprocess_bayer", "FrameLayout", "FrameAssembler", "FrameSynthesizer",
           "PhysicsNoiseBatchBuilder", "CameraNoiseModel", "physics_frames", "tukey_lambda_quantile",
           "DarkStack", "calibrate_dark_frames", "table_row", "ppcc_max", "probplot", "__version__"]


def __getattr__(name):
    # lazy: importing the package must not require torch.cuda or the built library
    if name == "GaussianDiffusion":
        from .diffusion import GaussianDiffusion
        return GaussianDiffusion
    if name in ("NoiseDiffNet", "UNet_PosEmbV2", "UNet_PosEmbV2_NoPosition", "UNet_PosEmbV2_CameraCond"):
        from . import net
        return getattr(net, name)
    if name == "LSID":
        from .lsid import LSID
        return LSID
    if name == "TrainableNoiseDiffNet":
        from .trainable import TrainableNoiseDiffNet
        return TrainableNoiseDiffNet
    if name == "TrainableLSID":
        from .lsid_train import TrainableLSID
        return TrainableLSID
    if name in ("pack_raw", "load_pair", "to_bayer", "RealBatchBuilder", "PoissonGaussianBatchBuilder"):
        from . import raw
        return getattr(raw, name)
    if name in ("DiffusionBatchBuilder", "GenerationBatchBuilder", "balanced_sample_list"):
        from . import diffusion_data
        return getattr(diffusion_data, name)
    if name in ("kld_edges", "get_histogram", "histogram_counts", "kl_div_forward", "kl_div_inverse", "kl_div_sym", "kl_div_3", "noise_kld",
                "patch_std_mean", "poisson_lambda_by_patch"):
        from . import noise_stats
        return getattr(noise_stats, name)
    if name in ("LevelMoments", "level_curve", "theil_sen", "get_poisson_lambda", "get_poisson_lambda_all_images",
                "get_regression_result_all_images"):
        from . import noise_level
        return getattr(noise_level, name)
    if name in ("Develop", "gamma_curve", "postprocess_bayer"):
        from . import render
        return getattr(render, name)
    if name in ("FrameLayout", "FrameAssembler", "FrameSynthesizer"):
        from . import frame
        return getattr(frame, name)
    if name in ("PhysicsNoiseBatchBuilder", "CameraNoiseModel", "physics_frames", "tukey_lambda_quantile"):
        from . import physics_noise
        return getattr(physics_noise, name)
    if name in ("DarkStack", "calibrate_dark_frames", "table_row", "ppcc_max", "probplot"):
        from . import calibrate
        return getattr(calibrate, name)
    raise AttributeError(name)
