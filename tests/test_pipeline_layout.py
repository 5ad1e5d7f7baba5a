"""Where the detection pipeline lives (camouflage_multimodal_amd/pipeline.py): the two things its entry points share
-- the group-by-size loop and the choice of ``match``'s ground-truth ids -- on the host, and the layering of the modules around it,
read off the source files with ``ast``.  No device and no library: the branches that launch kernels are held by the
tests/test_*_pipeline.py files.
"""
import ast
import os

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "camouflage_multimodal_amd")
LAYERED = ("resize.py", "rg_detect.py", "refine.py", "rg_finetune.py", "pipeline.py", "instance_match.py")
PUBLIC = {"decode_polygon_arrays", "decode_polygons", "polygons_to_rles", "decode_segmentations", "coco_ground_truth", "label_runs",
          "rles_from_runs", "encode_instances", "decode_rles", "counts_to_string", "string_to_counts", "rle_area", "match_instances",
          "instance_match_records", "InstanceAP", "guided_filter", "guided_upsample", "mask_instances", "instance_records", "detect_instances",
          "pack_images", "resize_batch", "resize_to_sizes", "random_resized_crops", "RaggedImages", "detect_camouflage_ragged",
          "prepare_finetune_batch_ragged", "detect_camouflage_directory", "segmentation_histograms", "cod_measures", "weighted_f_measure",
          "aggregate_cod_measures", "node_targets_from_masks", "prepare_finetune_batch", "RegionGraphFineTuner", "FineTuneBatch",
          "detect_camouflage", "detect_camouflage_batch", "paint_regions", "attention_to_pixels", "segmentation_counts", "segmentation_metrics",
          "RegionGraphGNN", "RegionGraphData", "RegionGraphBatch", "create_region_graphs_from_segments", "region_graphs_from_images",
          "slic_label_bound", "predict_batch_from_images", "create_region_graph", "create_region_graph_from_segments", "canny_edges",
          "slic_segments", "region_graph_from_image", "predict_from_image", "build_target_csr", "build_multimodal_model",
          "MultimodalCamouflageDetector", "CrossAttentionFusion", "LateFusion", "AggressiveFocalLoss", "multitask_loss", "FusedClipAdamW",
          "cosine_warm_restarts_lr", "NativeTrainer", "calculate_f1_score", "collate_fn", "fit", "pack_samples", "train_epoch_fixed",
          "validate_fixed", "EmbeddingMatcher", "DeviceResidentDataset", "SmartMultimodalDataset", "extract_label_from_mask",
          "train_multimodal_fixed", "load_multimodal_model", "build_ordered_kg_tensor", "predict_from_embeddings",
          "predict_batch_from_embeddings", "predict_from_region_graph", "predict_embedding_directory"}


def test_groups_by_size_in_first_appearance_order_and_scatters_back():
    from camouflage_multimodal_amd.pipeline import _by_size
    shapes = [(4, 6), (8, 2), (4, 6), (3, 3), (8, 2)]
    calls = []

    def one(idx, size):
        calls.append((list(idx), size))
        return [(i, size) for i in idx]

    assert _by_size(shapes, one) == [(i, s) for i, s in enumerate(shapes)]
    assert calls == [([0, 2], (4, 6)), ([1, 4], (8, 2)), ([3], (3, 3))]

    calls.clear()

    def three(idx, size):
        calls.append((list(idx), size))
        return [i for i in idx], [10 * i for i in idx], {j: size for j in range(len(idx))}      # (anything indexable by 0 .. len - 1)

    a, b, c = _by_size(shapes, three, 3)
    assert (a, b, c) == ([0, 1, 2, 3, 4], [0, 10, 20, 30, 40], shapes)
    assert calls == [([0, 2], (4, 6)), ([1, 4], (8, 2)), ([3], (3, 3))]

    class Shaped:                                    # (a tensor is taken by its shape)
        def __init__(self, *shape):
            self.shape = shape

    assert _by_size([Shaped(*s) for s in shapes], lambda idx, size: [size] * len(idx)) == shapes


def test_grouping_nothing_calls_nothing():
    from camouflage_multimodal_amd.pipeline import _by_size

    def never(idx, size):
        raise AssertionError("called for an empty input")

    assert _by_size([], never) == []
    assert _by_size([], never, 1) == ([],)
    assert _by_size([], never, 3) == ([], [], [])


@pytest.mark.parametrize("noun", ["images", "files"])
def test_ground_truth_ids_given_as_maps(noun):
    from camouflage_multimodal_amd.instance_match import match_options
    from camouflage_multimodal_amd.pipeline import _match_ground_truth
    maps = [object(), object(), object()]
    opts = match_options({"gt_labels": maps})
    sizes = [(4, 6), (8, 2), (4, 6)]
    assert _match_ground_truth(opts, 3, noun, sizes, None, 8, None) is maps      # (untouched: no device, no masks, no call)
    with pytest.raises(ValueError, match=rf'^match\["gt_labels"\] holds 3 maps for 2 {noun}$'):
        _match_ground_truth(opts, 2, noun, sizes[:2], None, 8, None)


def _relative_imports(name):
    """(module-level relative imports as {module or name}, relative imports inside a function or method) of a package file."""
    tree = ast.parse(open(os.path.join(PKG, name)).read())
    top, inner = set(), []

    def names(node):
        return {node.module.split(".")[0]} if node.module else {a.name for a in node.names}

    for node in tree.body:
        if isinstance(node, ast.ImportFrom) and node.level:
            top |= names(node)
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
            for node in ast.walk(fn):
                if isinstance(node, ast.ImportFrom) and node.level:
                    inner.append((getattr(fn, "name", "lambda"), sorted(names(node))))
    return top, inner


@pytest.mark.parametrize("name", LAYERED)
def test_no_package_import_inside_a_function(name):
    assert _relative_imports(name)[1] == []


def test_the_bindings_do_not_import_what_runs_on_them():
    assert _relative_imports("resize.py")[0] <= {"_lib", "engine"}
    assert _relative_imports("rg_detect.py")[0] <= {"_lib", "engine", "region_graph"}
    top = _relative_imports("pipeline.py")[0]
    assert "rg_finetune" not in top
    assert {"resize", "rg_detect", "refine", "instances", "instance_match", "rle", "polygons", "seg_measures", "region_graph"} <= top
    for name in top - {"_lib", "engine"}:                                     # nothing the pipeline imports imports the trainer or the pipeline
        assert not _relative_imports(name + ".py")[0] & {"rg_finetune", "pipeline"}, name


def test_public_surface_is_what_it_was():
    import camouflage_multimodal_amd as pkg
    assert set(pkg.__all__) == PUBLIC and len(pkg.__all__) == len(PUBLIC)
    assert all(hasattr(pkg, name) for name in PUBLIC)
    for name in ("detect_camouflage", "detect_camouflage_batch", "detect_camouflage_ragged", "detect_camouflage_directory"):
        assert getattr(pkg, name).__module__ == "camouflage_multimodal_amd.pipeline"
        assert not hasattr(pkg.resize, name) and not hasattr(pkg.rg_detect, name)      # (no re-export left behind)
    assert pkg.prepare_finetune_batch_ragged.__module__ == "camouflage_multimodal_amd.rg_finetune"
