"""stain2stain_amd -- the stain-to-stain flow-matching hot path on MI355X (gfx950).

Drop-in replacements for the reference's torch-only network components (same signatures and
state_dict keys), computed by hand-written HIP kernels behind a C ABI
(include/stain2stain_hip.h, stain2stain_amd/csrc/*.hip).  HIP only: there is no CPU fallback.
"""
from .components import (ClassConditionalFlowUNet, FlowMatchingDecoder, FlowUNet, SegmentationDecoder, SharedEncoder,
                         TimeEmbedding)
from .flow_matching import (ClassConditionalFlowMatchingModule, ConditionalFlowMatcher,
                            ConditionalFlowMatchingModule, MaskConditionedFlowMatchingModule,
                            MultiTaskFlowMatchingModule, ROICharbonnierFlowMatchingModule,
                            GraphedVelocity, ROIWeightedFlowMatchingModule, SolverConfig, dopri5_generate, dopri5_integrate,
                            euler_generate, euler_integrate, FIXED_STEP_METHODS, fixed_step_generate,
                            fixed_step_integrate)
from . import checkpoint
from .pix2pix import (Conv4x4Stride1, Conv4x4Stride2, ConvTranspose4x4Stride2, InstanceNormLeakyReLU,
                      PatchGANDiscriminator, Pix2PixGenerator)
from .pix2pix_engine import Pix2PixTrainer
from .trainer import CFMTrainer
from .optim import FusedAdam
from .ema import FusedEMA
from .multitask_trainer import MultiTaskTrainer
from .evaluation import EvalAccumulator
from .region import multitask_sampler, plan_region_batches, plan_tiles, tissue_counts, translate_region
from .image_metrics import generation_quality, image_quality, plan_bands, region_quality
from .stain_quant import (region_stain_agreement, region_stain_map, stain_agreement, stain_matrix, stain_quantify,
                          stain_separate)
from .stain_calibrate import (calibrate_thresholds, match_thresholds, region_stain_histogram,
                              region_stain_pair_histogram, stain_histogram, stain_pair_histogram, stain_thresholds,
                              thresholds_tuple)
from .zonal import (distance_zones, object_zones, region_stain_zonal, region_stain_zonal_agreement, stain_zonal,
                    stain_zonal_agreement, stain_zonal_objects)
from .background import (concentration_bins, grey_morphology, region_stain_quantify_corrected,
                         stain_agreement_corrected, stain_background, stain_objects_corrected,
                         stain_quantify_corrected)
from .hysteresis import (clear_border, hysteresis_mask, hysteresis_thresholds, reconstruct_mask,
                         region_stain_objects_hysteresis, select_components, stain_agreement_hysteresis,
                         stain_objects_hysteresis)
from .stain_norm import REFERENCE_HE, StainFit, fit_stains, normalize_region, stain_normalize
from .objects import label_components, region_stain_objects, stain_object_agreement, stain_objects
from .augment import (PairedAugmenter, paired_augment, sample_d4_params, sample_stain_jitter, stain_augment,
                      stain_jitter_maps)
from .registration import (overlap_boxes, region_shift_field, register_pairs, registered_quality,
                           sample_crop_params_within, shift_tiles, structure_map, structure_weights)
from .warp import clean_shift_field, register_region, warp_region
from .rigid import (align_regions, register_rigid, rigid_transform, rigid_warp, rotation_table,
                    structure_overview)
from .qc import qc_keep, region_qc, region_qc_map, tile_qc, window_sums
from .morphology import distance_transform, fill_holes, mask_boundary, mask_boundary_agreement, mask_morphology
from .object_features import (object_feature_summary, object_features, region_stain_object_features,
                              stain_object_features)
from .split import label_agreement, split_objects, stain_object_split
from .render import (colormap, compare_regions, compose_panels, default_palette, downsample_region, render_classes,
                     render_heat, render_region)

__all__ = ["SharedEncoder", "FlowMatchingDecoder", "SegmentationDecoder", "TimeEmbedding", "FlowUNet",
           "ConditionalFlowMatcher", "ConditionalFlowMatchingModule", "MultiTaskFlowMatchingModule", "euler_generate", "dopri5_generate", "euler_integrate", "dopri5_integrate", "SolverConfig", "GraphedVelocity",
           "CFMTrainer", "ClassConditionalFlowUNet", "ClassConditionalFlowMatchingModule",
           "MaskConditionedFlowMatchingModule", "ROICharbonnierFlowMatchingModule", "ROIWeightedFlowMatchingModule",
           "checkpoint", "InstanceNormLeakyReLU", "Conv4x4Stride1", "Conv4x4Stride2", "ConvTranspose4x4Stride2",
           "Pix2PixGenerator", "PatchGANDiscriminator", "Pix2PixTrainer", "FusedAdam", "FusedEMA", "MultiTaskTrainer",
           "EvalAccumulator", "plan_tiles", "translate_region", "tissue_counts", "plan_region_batches", "multitask_sampler", "FIXED_STEP_METHODS",
           "fixed_step_generate", "fixed_step_integrate", "image_quality", "region_quality", "generation_quality",
           "plan_bands", "stain_matrix", "stain_quantify", "stain_agreement", "stain_separate", "region_stain_map",
           "region_stain_agreement", "fit_stains", "stain_normalize", "normalize_region", "StainFit", "REFERENCE_HE",
           "label_components", "stain_objects", "stain_object_agreement", "region_stain_objects",
           "paired_augment", "stain_augment", "stain_jitter_maps", "sample_d4_params", "sample_stain_jitter",
           "PairedAugmenter", "structure_weights", "structure_map", "register_pairs", "shift_tiles", "overlap_boxes",
           "sample_crop_params_within", "registered_quality", "region_shift_field",
           "clean_shift_field", "warp_region", "register_region",
           "structure_overview", "rigid_warp", "register_rigid", "align_regions", "rotation_table", "rigid_transform",
           "tile_qc", "region_qc", "region_qc_map", "qc_keep", "window_sums",
           "distance_transform", "mask_morphology", "fill_holes", "mask_boundary", "mask_boundary_agreement",
           "object_features", "stain_object_features", "region_stain_object_features", "object_feature_summary",
           "split_objects", "stain_object_split", "label_agreement",
           "render_classes", "render_heat", "compare_regions", "downsample_region", "render_region", "compose_panels",
           "default_palette", "colormap",
           "stain_histogram", "region_stain_histogram", "stain_thresholds", "calibrate_thresholds", "thresholds_tuple",
           "stain_pair_histogram", "region_stain_pair_histogram", "match_thresholds",
           "stain_zonal", "stain_zonal_agreement", "region_stain_zonal", "region_stain_zonal_agreement", "object_zones",
           "stain_zonal_objects", "distance_zones",
           "grey_morphology", "concentration_bins", "stain_background", "stain_quantify_corrected",
           "stain_objects_corrected", "stain_agreement_corrected", "region_stain_quantify_corrected",
           "select_components", "reconstruct_mask", "clear_border", "hysteresis_mask", "stain_objects_hysteresis",
           "stain_agreement_hysteresis", "region_stain_objects_hysteresis", "hysteresis_thresholds"]
