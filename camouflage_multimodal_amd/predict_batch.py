"""Batched prediction on top of the per-image inference surface of ``test_multimodal.py`` (which stays the reference's
``predict_single_image`` loop, unchanged): several images per model call, one device -> host copy per call.

In bf16 mode at the reference configuration the one call runs the fused inference schedule and takes its two head-averaged
attention maps from one extra launch (``fused_attention=True``, csrc/attn_maps.hip); in f32 mode the flag has no effect.
"""
from __future__ import annotations

import json
import os

import torch

from . import test_multimodal as _single
from .test_multimodal import batch_result_entry, build_ordered_kg_tensor


@torch.no_grad()
def predict_batch_from_embeddings(multimodal_model, rg_list, kg_embeddings_dict, device, return_attention=True):
    """``predict_from_embeddings`` for several images in ONE model call: ``rg_list`` holds every image's Region-Graph node embeddings
    [Nr_i, 128] (Nr may differ); they are packed, run through one ``forward_packed`` call, the [B, 6] outputs come to the host in
    one copy, and the reference's post-processing (test_multimodal.py:105-150 of the reference) runs per image on the host.
    Returns (list of the prediction dicts ``predict_from_embeddings`` returns, list of per-image attention maps
    {"rg2kg": [Nr_i, Nk], "kg2rg": [Nk, Nr_i]} on the device -- None without ``return_attention`` -- and the ordered KG dict)."""
    rg_list = [torch.as_tensor(r) for r in rg_list]
    if not rg_list:
        raise ValueError("predict_batch_from_embeddings needs at least one image")
    kg_tensor, kg_ordered = build_ordered_kg_tensor(kg_embeddings_dict)
    B = len(rg_list)
    nrs = [int(r.shape[0]) for r in rg_list]
    rg = torch.cat([r.reshape(r.shape[0], -1) for r in rg_list]).to(device)
    kg = kg_tensor.reshape(kg_tensor.shape[0], -1).to(device).unsqueeze(0).expand(B, -1, -1).contiguous()
    res = multimodal_model.forward_packed(rg, nrs, kg, return_attention=return_attention, fused_attention=True)
    mask_out, inst_out, edge_out, score_out = (t.float() for t in res[:4])
    C = mask_out.shape[1]
    host = torch.cat([mask_out, inst_out, edge_out, score_out], dim=1).cpu()          # the one device -> host copy
    mask_l, inst_l, edge_l, score = host[:, :C], host[:, C:2 * C], host[:, 2 * C], host[:, 2 * C + 1]
    mask_prob, inst_prob, edge_prob = torch.softmax(mask_l, dim=1), torch.softmax(inst_l, dim=1), torch.sigmoid(edge_l)
    mask_pred, inst_pred = mask_l.argmax(dim=1).tolist(), inst_l.argmax(dim=1).tolist()
    predictions = [{
        "mask_logits": mask_l[i:i + 1].clone(),
        "mask_prob": mask_prob[i:i + 1].clone(),
        "mask_pred": int(mask_pred[i]),
        "instance_prob": inst_prob[i:i + 1].clone(),
        "instance_pred": int(inst_pred[i]),
        "edge_prob": float(edge_prob[i]),
        "score": float(score[i]),
    } for i in range(B)]
    attn = None
    if return_attention and res[4] is not None:
        attn = [{"rg2kg": a1, "kg2rg": a2} for a1, a2 in zip(res[4]["rg2kg"], res[4]["kg2rg"])]
    return predictions, attn, kg_ordered


@torch.no_grad()
def predict_batch_from_images(multimodal_model, rg_model, images, kg_embeddings_dict, device, n_segments=500, return_attention=True):
    """``predict_from_image`` for a batch with no per-image step before the fusion model: superpixels, edge maps and region graphs
    of ``images`` [N, H, W, 3] float in [0, 1] in batched device calls (``region_graphs_from_images``), ONE
    ``extract_node_embeddings`` call on the block-diagonal graph, and the embeddings split by ``node_offsets`` (views) into
    ``predict_batch_from_embeddings``, whose result this returns.  Host synchronisations of the whole call: the graph sizes
    read-back and the final [N, 6] copy."""
    from .region_graph import region_graphs_from_images
    graphs, _ = region_graphs_from_images(images, n_segments, device)
    emb = rg_model.extract_node_embeddings(graphs)
    no = graphs.node_offsets
    return predict_batch_from_embeddings(multimodal_model, [emb[no[k]:no[k + 1]] for k in range(graphs.num_graphs)], kg_embeddings_dict, device,
                                         return_attention=return_attention)


def predict_embedding_directory(multimodal_model, rg_embeddings, kg_embeddings_dict, output_dir, device, max_images=None, batch_size=1):
    """``test_multimodal.predict_embedding_directory`` with a group size.  ``batch_size=1`` (default) IS that function: the
    per-image loop.  ``batch_size`` > 1: that many images per model call through ``predict_batch_from_embeddings`` (the attention
    maps, which this mode does not use, are not requested); same ``batch_results.json`` entries in the same order."""
    if batch_size <= 1:
        return _single.predict_embedding_directory(multimodal_model, rg_embeddings, kg_embeddings_dict, output_dir, device, max_images)
    os.makedirs(output_dir, exist_ok=True)
    results = []
    items = list(rg_embeddings.items())[:max_images]
    for g in range(0, len(items), batch_size):
        group = items[g:g + batch_size]
        preds, _, _ = predict_batch_from_embeddings(multimodal_model, [rg["node_embeddings"] for _, rg in group], kg_embeddings_dict,
                                                    device, return_attention=False)
        results.extend(batch_result_entry(name, pred) for (name, _), pred in zip(group, preds))
    with open(os.path.join(output_dir, "batch_results.json"), "w") as f:
        json.dump(results, f, indent=2)
    return results
