"""MI355X-native (gfx950) implementation of the camouflage-multimodal fusion hot path.

Public surface = the reference's operator API for this path:
``build_multimodal_model``, ``MultimodalCamouflageDetector`` (fusion_model.py),
``AggressiveFocalLoss``, ``calculate_f1_score``, ``train_epoch_fixed``, ``validate_fixed``
(train_multimodal.py), plus the native packed-batch trainer.  All arithmetic runs in
``libcamo_fusion.so`` (hand-written HIP, C ABI in include/camo_fusion.h); there is no CPU
fallback.
"""
from .embedding_matcher import DeviceResidentDataset, EmbeddingMatcher  # noqa: F401
from .fusion_model import (CrossAttentionFusion, LateFusion, MultimodalCamouflageDetector,  # noqa: F401
                           build_multimodal_model)
from .losses import AggressiveFocalLoss, multitask_loss  # noqa: F401
from .optim import FusedClipAdamW, cosine_warm_restarts_lr  # noqa: F401
from .test_multimodal import (build_ordered_kg_tensor, load_multimodal_model, predict_from_embeddings,  # noqa: F401
                              predict_from_region_graph)
# (the package's predict_embedding_directory is test_multimodal's with a group size: batch_size=1, the default, calls that one)
from .predict_batch import predict_batch_from_embeddings, predict_batch_from_images, predict_embedding_directory  # noqa: F401
from .train_multimodal import (NativeTrainer, SmartMultimodalDataset, calculate_f1_score, collate_fn,  # noqa: F401
                               extract_label_from_mask, fit, pack_samples, train_epoch_fixed, train_multimodal_fixed,
                               validate_fixed)

from .region_graph import (RegionGraphBatch, RegionGraphData, RegionGraphGNN, build_target_csr, canny_edges, create_region_graph,  # noqa: F401,E402
                           create_region_graph_from_segments, create_region_graphs_from_segments, predict_from_image,
                           region_graph_from_image, region_graphs_from_images, slic_label_bound, slic_segments)
from .rg_detect import attention_to_pixels, paint_regions, segmentation_counts, segmentation_metrics  # noqa: F401,E402
from .seg_measures import (aggregate_cod_measures, cod_measures, segmentation_histograms, weighted_f_measure)  # noqa: F401,E402
from .instances import detect_instances, instance_records, mask_instances  # noqa: F401,E402
from .instance_match import InstanceAP, instance_match_records, match_instances  # noqa: F401,E402
from . import boundary  # noqa: F401,E402  (Boundary IoU / Boundary AP: reached as camouflage_multimodal_amd.boundary.<name>)
from . import split  # noqa: F401,E402  (touching objects split at their necks: reached as camouflage_multimodal_amd.split.<name>)
from .refine import guided_filter, guided_upsample  # noqa: F401,E402
from .rle import (counts_to_string, decode_rles, encode_instances, label_runs, rle_area, rles_from_runs, string_to_counts)  # noqa: F401,E402
from .polygons import (coco_ground_truth, decode_polygon_arrays, decode_polygons, decode_segmentations, polygons_to_rles)  # noqa: F401,E402
from .resize import RaggedImages, pack_images, random_resized_crops, resize_batch, resize_to_sizes  # noqa: F401,E402
from .pipeline import detect_camouflage, detect_camouflage_batch, detect_camouflage_directory, detect_camouflage_ragged  # noqa: F401,E402
from .rg_finetune import (FineTuneBatch, RegionGraphFineTuner, node_targets_from_masks, prepare_finetune_batch,  # noqa: F401,E402
                          prepare_finetune_batch_ragged)

__all__ = ["decode_polygon_arrays", "decode_polygons", "polygons_to_rles", "decode_segmentations", "coco_ground_truth", "label_runs", "rles_from_runs", "encode_instances", "decode_rles", "counts_to_string", "string_to_counts", "rle_area", "match_instances", "instance_match_records", "InstanceAP", "guided_filter", "guided_upsample", "mask_instances", "instance_records", "detect_instances", "pack_images", "resize_batch", "resize_to_sizes", "random_resized_crops", "RaggedImages", "detect_camouflage_ragged", "prepare_finetune_batch_ragged", "detect_camouflage_directory",
           "segmentation_histograms", "cod_measures", "weighted_f_measure", "aggregate_cod_measures","node_targets_from_masks", "prepare_finetune_batch", "RegionGraphFineTuner", "FineTuneBatch", "detect_camouflage", "detect_camouflage_batch", "paint_regions", "attention_to_pixels", "segmentation_counts", "segmentation_metrics", "RegionGraphGNN", "RegionGraphData", "RegionGraphBatch", "create_region_graphs_from_segments", "region_graphs_from_images", "slic_label_bound", "predict_batch_from_images", "create_region_graph", "create_region_graph_from_segments", "canny_edges", "slic_segments", "region_graph_from_image", "predict_from_image", "build_target_csr", "build_multimodal_model", "MultimodalCamouflageDetector", "CrossAttentionFusion", "LateFusion",
           "AggressiveFocalLoss", "multitask_loss", "FusedClipAdamW", "cosine_warm_restarts_lr", "NativeTrainer",
           "calculate_f1_score", "collate_fn", "fit", "pack_samples", "train_epoch_fixed", "validate_fixed",
           "EmbeddingMatcher", "DeviceResidentDataset", "SmartMultimodalDataset", "extract_label_from_mask", "train_multimodal_fixed", "load_multimodal_model", "build_ordered_kg_tensor",
           "predict_from_embeddings", "predict_batch_from_embeddings", "predict_from_region_graph", "predict_embedding_directory"]
