"""Host-side mirror of the reference's model driver (/root/reference/src/tf_aerial_images.py:51-379):
`Options` (the 30 flags) and `ConvolutionalModel` with train / predict / predict_batchwise / save / restore -- same names,
argument meaning, batch/tiling conventions and quirks that matter for parity -- over the HIP path (unet.UNet).

Data parallelism (new; the reference is single-device): when torch.distributed is initialised, `batch_size` is the GLOBAL
minibatch, sharded contiguously over ranks; gradients are all-reduced (dist.GradBucketer); predict() shards tiles.
"""
import contextlib
import glob
import math
import os
from datetime import datetime

import numpy as np
import torch
import torch.distributed as dist

from . import hostio
from . import images as dimages
from . import mask_metrics
from ._lib import call
from .hostio import GRAPH_MAX_BRANCH, SEGMENTS_MAX_EDGES, SEGMENTS_MAX_SIDE, THIN_MAX_ITERS, THIN_MAX_SIDE
from .hostio import road_graph as hostio_road_graph
from .hostio import PATHS_MAX_LEN, PATHS_MAX_SIDE, simplify_path
from .hostio import ROUTES_INF, ROUTES_MAX_NODES, ROUTES_MAX_SIDE
from .dist import GradBucketer, micro_indices, shard_indices, tune_overlap  # noqa: F401  (shard_indices: importable from here as before)
from .pool import BatchUploader, DevicePatchPool, PatchPool
from .summary import Summary
from .unet import DECAY_MODES, EMA_SUFFIX, LR_SCHEDULES, UNet, input_size_needed

# (name, type, default, help) -- tf_aerial_images.py:15-46, same order
FLAG_DEFS = [
    ("batch_size", int, 25, "Batch size of training instances"),
    ("dilated_layers", bool, False, "Add dilated CNN layers"),
    ("dropout", float, 0.8, "Probability to keep an input"),
    ("ensemble_prediction", bool, False, "Ensemble Prediction"),
    ("eval_data_dir", str, None, "Directory containing eval images"),
    ("eval_every", int, 500, "Number of steps between evaluations"),
    ("eval_train", bool, False, "Evaluate training data"),
    ("gpu", int, -1, "GPU to run the model on"),
    ("image_augmentation", bool, False, "Augment training set of images with transformations"),
    ("interactive", bool, False, "Spawn interactive Tensorflow session"),
    ("logdir", str, os.path.abspath("./logdir"), "Directory where to write logfiles"),
    ("lr", float, 0.01, "Initial learning rate"),
    ("model_path", str, None, "Restore exact model path"),
    ("momentum", float, 0.9, "Momentum"),
    ("num_epoch", int, 5, "Number of pass on the dataset during training"),
    ("num_eval_images", int, 4, "Number of images to predict for an evaluation"),
    ("num_gpu", int, 1, "Number of available GPUs to run the model on"),
    ("num_layers", int, 5, "Number of layers of the U-Net"),
    ("patch_size", int, 128, "Size of the prediction image"),
    ("pred_batch_size", int, 2, "Batch size of batchwise prediction"),
    ("restore_date", str, None, "Restore the model from specific date"),
    ("restore_epoch", int, None, "Restore the model from specific epoch"),
    ("restore_model", bool, False, "Restore the model from previous checkpoint"),
    ("root_size", int, 64, "Number of filters of the first U-Net layer"),
    ("rotation_angles", str, None, "Rotation angles"),
    ("save_path", str, os.path.abspath("./runs"), "Directory where to write checkpoints, overlays and submissions"),
    ("seed", int, 2017, "Random seed for reproducibility"),
    ("stride", int, 16, "Sliding delta for patches"),
    ("train_data_dir", str, os.path.abspath("./data/training"), "Directory containing training images/ groundtruth/"),
    ("train_score_every", int, 1000, "Compute training score after the given number of iterations"),
]


# options the reference does not have (kept apart from its 30 flags): where the training patches live and the D4 augmentation
EXTRA_FLAG_DEFS = [
    ("device_patch_pool", bool, True, "Keep the rotated training images in HBM and cut the patches of a batch on the GPU"),
    ("d4_augmentation", bool, False, "Stochastic flips / transpose / rot90 per training sample on the GPU (what the reference's "
                                     "--image_augmentation subgraph intended; that flag itself stays without effect, as in the reference)"),
    ("optimizer", str, "momentum", "momentum|adam: the reference's MomentumOptimizer (--lr, --momentum) or tf.train.AdamOptimizer (--lr, "
                                   "--adam_beta1, --adam_beta2, --adam_epsilon; --lr keeps the reference's default 0.01, TensorFlow's Adam default is 0.001)"),
    ("adam_beta1", float, 0.9, "Adam: decay rate of the first-moment estimates"),
    ("adam_beta2", float, 0.999, "Adam: decay rate of the second-moment estimates"),
    ("adam_epsilon", float, 1e-8, "Adam: epsilon added to sqrt(v)"),
    ("class_weights", str, None, "Loss weights of the classes background,road: 'w0,w1' (two finite floats >= 0, not both 0) or 'balanced' "
                                 "(N / (2 N_c) from the training ground truth: mean weight 1, so --lr keeps its scale); default: the "
                                 "reference's unweighted loss. The loss stays normalised by the pixel count, not by the sum of the weights"),
    ("dice_weight", float, 0.0, "lambda >= 0 of a soft-Dice (soft-F1) term: loss = cross-entropy + lambda * (1 - Dice), Dice over each GPU's "
                                "batch; 0 = off (the reference's loss). Ignored pixels and the weight map enter Dice, class weights do not"),
    ("dice_smooth", float, 1.0, "Smoothing constant s > 0 of Dice = (2 I + s) / (P + Y + s)"),
    ("focal_gamma", float, 0.0, "gamma >= 0 (finite) of the focal loss (Lin et al. 2017): every pixel's cross-entropy counts (1 - p_t)^gamma "
                                "times, p_t the probability of its true class; 0 = off (2 is the paper's choice). The logged loss and the "
                                "validation loss / objective are then the focal objective. The gradient shrinks with gamma (the loss stays "
                                "normalised by the pixel count), so --lr needs retuning. It multiplies --class_weights, --border_weight and "
                                "the weight map; --dice_weight adds to it unchanged"),
    ("cldice_weight", float, 0.0, "lambda >= 0 of a clDice (centre-line Dice, Shit et al. 2021) term: loss += lambda * (1 - clD), clD over each "
                                  "GPU's batch from the soft skeletons of the prediction and of the labels; 0 = off. It sees connectivity, "
                                  "which no per-pixel or overlap term does. Ignored pixels add nothing to it; --class_weights, the weight "
                                  "maps and --focal_gamma do not enter it"),
    ("cldice_iters", int, 10, "Erosions k of the soft skeleton, an int in [0, 16]: at least the half-width, in pixels, of the widest road"),
    ("cldice_smooth", float, 1.0, "Smoothing constant s > 0 of the clDice ratios (A + s) / (Bp + s) and (Cc + s) / (Dy + s)"),
    ("lovasz_weight", float, 0.0, "lambda >= 0 of a Lovasz (Jaccard surrogate, Berman et al. 2018) term: loss += lambda * the mean over the "
                                  "images of the per-image Lovasz loss of |label - p|, a convex surrogate of 1 - IoU; 0 = off. A mean of "
                                  "per-image losses: data-parallel and accumulated steps give the objective of one large batch. Ignored "
                                  "pixels add nothing to it; --class_weights, the weight maps and --focal_gamma do not enter it"),
    ("min_road_area", int, 0, "A >= 0: remove predicted road components (pixels with probability >= the threshold, joined at "
                              "--component_connectivity) of fewer than A pixels before the masks are quantised or binarised, on the GPU "
                              "(rsu_components.h); 0 = off. Applies to the inference and --eval_train branches and to postprocess_masks, "
                              "never to training"),
    ("max_hole_area", int, 0, "A >= 0: fill holes -- background regions of the cleaned mask, joined at the dual connectivity, that touch no "
                              "image edge -- of at most A pixels; runs after --min_road_area; 0 = off"),
    ("component_connectivity", int, 8, "4|8: the neighbourhood that joins road pixels into components; holes and background use the dual "
                                       "(4 for 8, 8 for 4)"),
    ("validate_components", bool, False, "Count connected components during validation: evaluate() also returns components_pred, "
                                         "components_true and b0_error, the mean over the validation patches of |predicted - true| "
                                         "component counts (the error of the zeroth Betti number) at --component_connectivity"),
    ("validate_distances", bool, False, "Measure distances during validation: evaluate() also returns dist_hist (the predicted road pixels "
                                        "by their distance to the nearest true road pixel and the other way round, on the GPU: "
                                        "rsu_distance.h) and from it the buffer-relaxed relaxed_precision, relaxed_recall and relaxed_f1 "
                                        "of Mnih & Hinton at --relaxed_slack, mean_dist_pred / mean_dist_true and far_pred / far_true. "
                                        "Distances are per validation patch: a true road just outside the patch is not seen"),
    ("relaxed_slack", int, 3, "RHO, an int in [0, 62]: a predicted road pixel counts as correct when a true road pixel lies within RHO "
                              "pixels, and a true one as found when a predicted one does (3 on the Massachusetts roads set; 0 = the plain "
                              "pixel precision and recall). Used with --validate_distances"),
    ("save_best_metric", str, "f1", "f1|relaxed_f1|cl_quality|apls: the validation figure --save_best compares; apls requires "
                                    "--validate_routes; relaxed_f1 requires "
                                    "--validate_distances, cl_quality requires --validate_centerlines"),
    ("validate_centerlines", bool, False, "Extract centre-lines during validation: evaluate() thins the predicted and the true road mask "
                                          "of every patch to one-pixel skeletons on the GPU (Guo & Hall's parallel thinning: "
                                          "rsu_thin.h) and also returns cl_hist (the distance histogram of the two skeletons) and from "
                                          "it cl_correctness, cl_completeness and cl_quality (Wiedemann, Heipke) at --relaxed_slack, "
                                          "cldice_hard (the clDice metric on hard skeletons), cl_len_pred / cl_len_true (skeleton pixel "
                                          "counts) and thin_unconverged. Skeletons are per validation patch. Does not need "
                                          "--validate_distances"),
    ("centerline_max_iters", int, 64, "Thinning iterations at most, an int in [1, 512]: a road of half-width w needs about w + 6; image "
                                      "sides still changing after them are counted in thin_unconverged. Used by --validate_centerlines "
                                      "and --save_centerlines"),
    ("save_centerlines", bool, False, "Inference: also write the centre-line of every predicted mask (after --min_road_area / "
                                      "--max_hole_area, at threshold 0.5) as a greyscale PNG beside the overlays"),
    ("centerline_min_branch", int, 0, "L, an int in [0, 64]: prune the centre-lines on the GPU (morphological pruning: rsu_graph.h); a "
                                      "branch of at most L pixels is removed, a longer one kept whole; 0 = off. Used by "
                                      "--validate_centerlines (cl_hist, cl_correctness, cl_completeness, cl_quality, cl_len_pred and "
                                      "cl_len_true then describe the pruned centre-lines; cldice_hard stays on the unpruned skeletons, its "
                                      "counts need the full masks, which only the thinning sees) and --save_centerlines. A spur within L "
                                      "pixels of a true line end returns with that end"),
    ("validate_junctions", bool, False, "Requires --validate_centerlines: evaluate() also marks the junction pixels, ends and isolated "
                                        "pixels of both (pruned) centre-lines on the GPU and returns jn_hist (the distance histogram of "
                                        "the two junction-pixel masks), jn_precision, jn_recall and jn_f1 at --relaxed_slack, "
                                        "junctions_pred / junctions_true (8-connected clusters of junction pixels), junction_error (the "
                                        "mean |predicted - true| clusters per patch), ends_pred / ends_true and isolated_pred / "
                                        "isolated_true. A road that leaves its patch ends there and counts as an end on both sides "
                                        "alike: the comparison is the figure, not the count"),
    ("validate_segments", bool, False, "Requires --validate_centerlines: evaluate() also cuts both (pruned) centre-lines at their "
                                       "junctions into road segments on the GPU (rsu_segments.h) and returns segments_pred / segments_true, "
                                       "road_length_pred / road_length_true (orthogonal links + sqrt(2) diagonal links, from node zone to "
                                       "node zone), seg_len_mean_*, dangling_*, free_*, rings_*, multi_*, segments_dropped_* (segments "
                                       "past --max_segments in a patch), nodes_* and length_ratio. Segments are per validation patch: a "
                                       "road that leaves its patch ends there"),
    ("max_segments", int, 4096, "An int in [1, 65536]: the rows of the segment table per image and side. Segments past it are counted "
                                "(segments_dropped_*) but not measured. Used by --validate_segments and --save_road_graph"),
    ("validate_routes", bool, False, "Requires --validate_segments: evaluate() also measures both road networks as networks on the GPU "
                                     "(rsu_routes.h): the length of the shortest path between every two nodes (junction zones and line "
                                     "ends) of each graph, and the average path length similarity of Van Etten et al. with those nodes as "
                                     "control points: apls_true_to_pred, apls_pred_to_true, apls (their harmonic mean), route_pairs_*, "
                                     "route_unmatched_*, route_broken_*, graph_nodes_* and graph_nodes_dropped_* (nodes past "
                                     "--max_graph_nodes in a patch). No points are injected along the edges; everything is per patch"),
    ("max_graph_nodes", int, 256, "An int in [1, 1024]: the rows of the node table per image and side, and the side of its distance "
                                  "matrix. Nodes past it are counted (graph_nodes_dropped_*) and their edges skipped. Used by "
                                  "--validate_routes and --road_graph_distances"),
    ("route_snap", int, 8, "An int in [0, 1023]: the pixels within which a node of one graph finds its counterpart in the other "
                           "(--validate_routes). A junction's centroid moves by a few pixels between a prediction and the truth, so "
                           "--relaxed_slack's 3 is too tight here; 8 is a choice, not a measurement"),
    ("save_road_graph", bool, False, "Inference: also write the road network of every predicted mask (after --min_road_area / "
                                     "--max_hole_area, at threshold 0.5; thinned, pruned by --centerline_min_branch, cut into segments) "
                                     "as graph_%03d.json beside the overlays: nodes (junctions, ends, isolated pixels) and edges with "
                                     "their lengths"),
    ("road_graph_paths", bool, False, "With --save_road_graph (and road_graph()): also order the pixels of every segment along it on the "
                                      "GPU (rsu_paths.h) and give every edge its \"kind\" (open | ring | branched | long) and its \"path\", a "
                                      "list of [y, x] from node a to node b where that is decidable; branched and long segments get an "
                                      "empty path, and every graph their number as \"unordered\""),
    ("max_path_length", int, 4096, "An int in [1, 1048576]: segments of more pixels are not ordered (kind \"long\"). Used by "
                                   "--road_graph_paths"),
    ("road_graph_simplify", float, 0.0, "EPS >= 0: simplify every path of --road_graph_paths with Ramer-Douglas-Peucker at EPS pixels (the "
                                        "first and last point stay); 0 = every pixel"),
    ("road_graph_distances", bool, False, "With --save_road_graph (and road_graph()): also give every graph \"node_index\", its node ids in "
                                          "the order of the GPU's node table (rsu_routes.h, --max_graph_nodes rows), and \"distances\", the "
                                          "length in pixels of the shortest path between every two of them, row-major over node_index, "
                                          "null where there is no path"),
    ("border_weight", float, 0.0, "w0 >= 0 of a border-distance weight map computed on the GPU from each batch's labels: a pixel counts "
                                  "1 + w0 * exp(-d^2 / (2 border_sigma^2)) times in the loss, d its distance to the other class inside its patch; "
                                  "0 = off (the U-Net paper uses 10). The loss stays normalised by the pixel count and the mean weight is above 1, "
                                  "so the effective step size rises with w0: retune --lr. It multiplies --class_weights and enters the Dice term"),
    ("border_sigma", float, 5.0, "Width sigma > 0, in pixels, of the border weight (the U-Net paper uses 5)"),
    ("clip_grad_norm", float, 0.0, "Clip the gradient to this global L2 norm (over all variables, after the data-parallel average) before the "
                                   "optimizer step, and skip a step whose gradient is not finite; 0 = off. Computed on the GPU without a host "
                                   "synchronisation; grad_norm is logged per step and the clipped / skipped counts per epoch. A huge value "
                                   "(1e30) only measures and guards"),
    ("validation_images", int, 0, "Hold out the last K training images, whole, as a validation set (0 = off); K must leave at least one "
                                  "training image, and --class_weights=balanced counts the remaining images only"),
    ("validate_every", int, 0, "Number of steps between validations on the held-out images; 0 = once at the end of each epoch"),
    ("save_best", bool, False, "Keep <save_path>/<experiment>-best.chkpt, rewritten whenever the validation F1 (--save_best_metric) improves"),
    ("ema_decay", float, 0.0, "Decay d (0 <= d < 1) of an exponential moving average of the weights, tf.train.ExponentialMovingAverage, "
                              "updated on the GPU after every optimizer step; 0 = off. Validation, --save_best, prediction and the final "
                              "inference then use the averaged weights; checkpoints hold both the raw weights and the averages"),
    ("ema_warmup", bool, True, "TensorFlow's num_updates rule for --ema_decay: the decay of update t is min(d, (1 + t) / (10 + t))"),
    ("random_rotation", float, 0.0, "Rotate every training sample by a random angle in [-DEG, DEG] degrees (finite, >= 0; 0 = off; 180 = any "
                                    "orientation), bilinear, mirrored at the image's edges, on the GPU as the batch is cut: no further copy of "
                                    "the training set. Needs --device_patch_pool; composes with --d4_augmentation and --random_scale"),
    ("random_scale", str, "1,1", "LO,HI: zoom every training sample by a random log-uniform factor in [LO, HI] (1/64 < LO <= HI <= 64; "
                                 "1,1 = off), in the same launch as --random_rotation. Needs --device_patch_pool"),
    ("one_launch_loader", bool, False, "Cut plain and --d4_augmentation batches with the one-launch loader kernel too: the bits of the "
                                       "per-sample copies it replaces for unrotated images; in the border band of a --rotation_angles copy "
                                       "it shows the mirror of the image instead of rotated content. Needs --device_patch_pool"),
    ("color_jitter", str, "0,0,0,0", "B,C,S,H: per training sample, on the GPU behind the loader, a random brightness factor in [1-B, 1+B], "
                                     "contrast factor in [1-C, 1+C] about the sample's own channel means, saturation factor in [1-S, 1+S] "
                                     "and hue rotation in [-H, H] degrees (B, C, S in [0, 1), H in [0, 180]; 0,0,0,0 = off), clamped to "
                                     "[0, 1] once at the end. Needs --device_patch_pool; labels and geometric draws do not change"),
    ("random_noise", float, 0.0, "SIGMA in [0, 1]: add per-element noise of standard deviation SIGMA (a sum of four uniforms, a key per "
                                 "sample) to every training sample, in the same pass as --color_jitter; 0 = off. Needs --device_patch_pool"),
    ("elastic_deformation", str, "0,3", "ALPHA,GRID: bend every training sample by a smooth random displacement field, the U-Net paper's "
                                        "elastic deformation, inside the one-launch loader kernel: control points of standard deviation "
                                        "ALPHA pixels (0 <= ALPHA <= 64; 0 = off) on a lattice of GRID cells per axis across the input "
                                        "window (an integer, 1..16), interpolated by a cubic B-spline; labels move with the image. The "
                                        "interpolated field's deviation is smaller than ALPHA; a large ALPHA on a fine GRID can fold the "
                                        "field. Needs --device_patch_pool; composes with --random_rotation, --random_scale and "
                                        "--d4_augmentation"),
    ("accumulate_steps", int, 1, "K >= 1: take one optimizer step over K micro-batches, summing their gradients on the GPU; 1 = off. "
                                 "--batch_size stays the effective (global) batch of one optimizer step and must divide by GPUs x K: "
                                 "each GPU runs K passes over batch_size / (GPUs x K) patches, so the 2-GiB limit on a batch applies to "
                                 "the micro-batch. Steps, --eval_every and the learning-rate decay count optimizer steps. The Dice term "
                                 "(--dice_weight) is taken per micro-batch, as it is per GPU, and dropout draws new masks per micro-batch"),
    ("weight_decay", float, 0.0, "lambda >= 0 (finite) of a weight decay applied inside the optimizer's update launch, at no extra pass over "
                                 "the weights; 0 = off. The 3x3, first and transposed conv kernels decay; biases, the colour-adjust matrix "
                                 "and the 1x1 head do not. The reported loss never includes the L2 penalty"),
    ("weight_decay_mode", str, "decoupled", "decoupled|l2: decoupled (AdamW; the same step in front of the Momentum rule) takes lr * lambda * w "
                                            "off every decaying weight at the scheduled rate; l2 adds lambda * w to its gradient, behind "
                                            "--clip_grad_norm's factor (the penalty lambda / 2 |w|^2)"),
    ("lr_schedule", str, "staircase", "staircase|constant|cosine|linear: the learning-rate curve over optimizer steps. staircase is the "
                                      "reference's lr * 0.95 ^ (step // 1000); cosine and linear fall from --lr to --lr_final * lr over "
                                      "--lr_total_steps steps and stay there"),
    ("lr_warmup_steps", int, 0, "W >= 0: scale the rate of step t by min(1, (t + 1) / W), a linear ramp over the first W optimizer steps, on "
                                "top of any --lr_schedule; 0 = off"),
    ("lr_total_steps", int, 0, "T >= 0: the horizon of --lr_schedule=cosine|linear in optimizer steps; 0 = this run's own length, --num_epoch "
                               "times the optimizer steps of an epoch (printed once the patches are known)"),
    ("lr_final", float, 0.0, "F in [0, 1]: the fraction of --lr at which --lr_schedule=cosine|linear end"),
]


def parse_class_weights(value):
    """The --class_weights value: None -> None; "balanced" -> "balanced" (resolved from the training ground truth by the caller:
    balanced_class_weights); "w0,w1" or a pair of numbers -> (w0, w1) as floats. Anything else raises ValueError."""
    if value is None:
        return None
    if isinstance(value, str):
        if value.strip() == "balanced":
            return "balanced"
        parts = value.split(",")
    else:
        try:
            parts = list(value)
        except TypeError:
            parts = [value]
    try:
        cw = tuple(float(v) for v in parts)
    except (TypeError, ValueError):
        cw = ()
    if len(cw) != 2 or not all(math.isfinite(v) and v >= 0.0 for v in cw) or cw == (0.0, 0.0):
        raise ValueError("--class_weights must be 'w0,w1' (two finite floats >= 0, not both 0) or 'balanced', not %r" % (value,))
    return cw


def parse_dice_weight(value):
    """The --dice_weight value as a float: finite and >= 0 (0.0 = no Dice term). Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError("--dice_weight must be a finite float >= 0, not %r" % (value,))
    return v


def parse_focal_gamma(value):
    """The --focal_gamma value as a float: finite and >= 0 (0.0 = the plain cross-entropy). Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (math.isfinite(v) and v >= 0.0):
        raise ValueError("--focal_gamma must be a finite float >= 0, not %r" % (value,))
    return v


def focal_loss_terms(p1, labels, gamma, class_weights=None, pixel_weights=None):
    """The focal objective of include/rsu_loss.h recomputed on the host, in numpy float64, from road probabilities (a `predict` output or
    net.prob) and labels of the same shape: (sum omega F CE, sum omega) over the pixels whose label is 0 or 1 -- any other label ignores
    its pixel BY SELECTION, whatever its weight holds -- with p_t the probability of the pixel's label, F = (1 - p_t)^gamma, CE = -log p_t
    and omega = class_weights[label] * pixel_weights[pixel] (None: 1). A pixel with p_t == 0 has an infinite CE, as it has without the
    modulation; one with p_t == 1 adds 0. Divide the first sum by the pixel count for the logged `loss`, by the second for the weighted
    mean. gamma == 0 is the weighted cross-entropy."""
    gamma = parse_focal_gamma(gamma)
    p1, labels = np.asarray(p1, dtype=np.float64).reshape(-1), np.asarray(labels).reshape(-1)
    if p1.shape != labels.shape:
        raise ValueError("focal_loss_terms: %d probabilities, %d labels" % (p1.size, labels.size))
    valid = (labels == 0) | (labels == 1)
    lab = labels[valid].astype(np.int64)
    p_t = np.where(lab == 1, p1[valid], 1.0 - p1[valid])
    p_o = np.where(lab == 1, 1.0 - p1[valid], p1[valid])
    omega = np.ones(lab.size, np.float64) if class_weights is None else np.asarray(class_weights, np.float64)[lab]
    if pixel_weights is not None:
        pw = np.asarray(pixel_weights, dtype=np.float64).reshape(-1)
        if pw.shape != labels.shape:
            raise ValueError("focal_loss_terms: %d weights, %d labels" % (pw.size, labels.size))
        omega = omega * pw[valid]
    with np.errstate(divide="ignore"):
        ce = -np.log(p_t)
    F = np.power(p_o, gamma) if gamma > 0.0 else np.ones_like(p_o)
    terms = np.where(F == 0.0, 0.0, omega * F * ce)      # (p_t == 1: F = 0 and CE = 0)
    return float(terms.sum()), float(omega.sum())


def parse_cldice_weight(value):
    """The --cldice_weight value as a float: finite and >= 0 (0.0 = no clDice term). Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (math.isfinite(v) and v >= 0.0):
        raise ValueError("--cldice_weight must be a finite float >= 0, not %r" % (value,))
    return v


def parse_lovasz_weight(value):
    """The --lovasz_weight value as a float: finite and >= 0 (0.0 = no Lovasz term). Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (math.isfinite(v) and v >= 0.0):
        raise ValueError("--lovasz_weight must be a finite float >= 0, not %r" % (value,))
    return v


def parse_component_area(value, name="min_road_area"):
    """The --min_road_area / --max_hole_area value as an int >= 0 (0 = off; rsu_components.h takes a C int). Anything else raises
    ValueError."""
    try:
        v = int(value)
        ok = not isinstance(value, bool) and v == (float(value) if not isinstance(value, str) else v) and 0 <= v < (1 << 31)
    except (TypeError, ValueError, OverflowError):
        v, ok = 0, False
    if not ok:
        raise ValueError("--%s must be an integer >= 0, not %r" % (name, value))
    return v


def parse_component_connectivity(value):
    """The --component_connectivity value: 4 or 8 as an int. Anything else raises ValueError."""
    try:
        v = int(value)
        ok = not isinstance(value, bool) and v == (float(value) if not isinstance(value, str) else v) and v in (4, 8)
    except (TypeError, ValueError, OverflowError):
        v, ok = 0, False
    if not ok:
        raise ValueError("--component_connectivity must be 4 or 8, not %r" % (value,))
    return v


def parse_relaxed_slack(value):
    """The --relaxed_slack value as an int in [0, 62] (rsu_distance.h: bins 0 .. RSU_DIST_BINS - 2 are exact). Anything else raises
    ValueError."""
    try:
        v = int(value)
        ok = not isinstance(value, bool) and v == (float(value) if not isinstance(value, str) else v) and 0 <= v <= 62
    except (TypeError, ValueError, OverflowError):
        v, ok = 0, False
    if not ok:
        raise ValueError("--relaxed_slack must be an integer in [0, 62], not %r" % (value,))
    return v


def parse_save_best_metric(value):
    """The --save_best_metric value: "f1", "relaxed_f1", "cl_quality" or "apls". Anything else raises ValueError."""
    if not isinstance(value, str) or value not in ("f1", "relaxed_f1", "cl_quality", "apls"):
        raise ValueError("--save_best_metric must be f1, relaxed_f1 or cl_quality, or apls, not %r" % (value,))
    return value


def parse_centerline_max_iters(value):
    """The --centerline_max_iters value as an int in [1, 512] (rsu_thin.h RSU_THIN_MAX_ITERS). Anything else raises ValueError."""
    try:
        v = int(value)
        ok = not isinstance(value, bool) and v == (float(value) if not isinstance(value, str) else v) and 1 <= v <= THIN_MAX_ITERS
    except (TypeError, ValueError, OverflowError):
        v, ok = 0, False
    if not ok:
        raise ValueError("--centerline_max_iters must be an integer in [1, %d], not %r" % (THIN_MAX_ITERS, value))
    return v


def parse_centerline_min_branch(value):
    """The --centerline_min_branch value as an int in [0, 64] (rsu_graph.h RSU_GRAPH_MAX_BRANCH; 0 = off). Anything else raises
    ValueError."""
    try:
        v = int(value)
        ok = not isinstance(value, bool) and v == (float(value) if not isinstance(value, str) else v) and 0 <= v <= GRAPH_MAX_BRANCH
    except (TypeError, ValueError, OverflowError):
        v, ok = 0, False
    if not ok:
        raise ValueError("--centerline_min_branch must be an integer in [0, %d], not %r" % (GRAPH_MAX_BRANCH, value))
    return v


def parse_max_segments(value):
    """The --max_segments value as an int in [1, 65536] (rsu_segments.h RSU_SEGMENTS_MAX_EDGES). Anything else raises ValueError."""
    try:
        v = int(value)
        ok = not isinstance(value, bool) and v == (float(value) if not isinstance(value, str) else v) and 1 <= v <= SEGMENTS_MAX_EDGES
    except (TypeError, ValueError, OverflowError):
        v, ok = 0, False
    if not ok:
        raise ValueError("--max_segments must be an integer in [1, %d], not %r" % (SEGMENTS_MAX_EDGES, value))
    return v


def parse_max_graph_nodes(value):
    """The --max_graph_nodes value as an int in [1, 1024] (rsu_routes.h RSU_ROUTES_MAX_NODES). Anything else raises ValueError."""
    try:
        v = int(value)
        ok = not isinstance(value, bool) and v == (float(value) if not isinstance(value, str) else v) and 1 <= v <= ROUTES_MAX_NODES
    except (TypeError, ValueError, OverflowError):
        v, ok = 0, False
    if not ok:
        raise ValueError("--max_graph_nodes must be an integer in [1, %d], not %r" % (ROUTES_MAX_NODES, value))
    return v


def parse_route_snap(value):
    """The --route_snap value as an int in [0, 1023] (rsu_routes.h: slack). Anything else raises ValueError."""
    try:
        v = int(value)
        ok = not isinstance(value, bool) and v == (float(value) if not isinstance(value, str) else v) and 0 <= v <= 1023
    except (TypeError, ValueError, OverflowError):
        v, ok = 0, False
    if not ok:
        raise ValueError("--route_snap must be an integer in [0, 1023], not %r" % (value,))
    return v


def parse_max_path_length(value):
    """The --max_path_length value as an int in [1, 1048576] (rsu_paths.h RSU_PATHS_MAX_LEN). Anything else raises ValueError."""
    try:
        v = int(value)
        ok = not isinstance(value, bool) and v == (float(value) if not isinstance(value, str) else v) and 1 <= v <= PATHS_MAX_LEN
    except (TypeError, ValueError, OverflowError):
        v, ok = 0, False
    if not ok:
        raise ValueError("--max_path_length must be an integer in [1, %d], not %r" % (PATHS_MAX_LEN, value))
    return v


def parse_road_graph_simplify(value):
    """The --road_graph_simplify value as a finite float >= 0 (0 = every pixel). Anything else raises ValueError."""
    try:
        v = float(value)
        ok = not isinstance(value, bool) and np.isfinite(v) and v >= 0.0
    except (TypeError, ValueError, OverflowError):
        v, ok = 0.0, False
    if not ok:
        raise ValueError("--road_graph_simplify must be a finite number >= 0, not %r" % (value,))
    return v


def parse_cldice_iters(value):
    """The --cldice_iters value as an int in [0, 16] (rsu_cldice.h RSU_CLDICE_MAX_ITERS). Anything else raises ValueError."""
    try:
        v = int(value)
        ok = not isinstance(value, bool) and v == (float(value) if not isinstance(value, str) else v) and 0 <= v <= 16
    except (TypeError, ValueError):
        v, ok = 0, False
    if not ok:
        raise ValueError("--cldice_iters must be an int in [0, 16], not %r" % (value,))
    return v


def parse_cldice_smooth(value):
    """The --cldice_smooth value as a float: finite and > 0. Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (math.isfinite(v) and v > 0.0):
        raise ValueError("--cldice_smooth must be a finite float > 0, not %r" % (value,))
    return v


def cldice_from_sums(A, Bp, Cc, Dy, smooth):
    """clD = 2 Tp Ts / (Tp + Ts) with Tp = (A + s) / (Bp + s), Ts = (Cc + s) / (Dy + s), from the sums A = sum m skel(p) y, Bp = sum m skel(p),
    Cc = sum m skel(y) p, Dy = sum m skel(y) that rsu_cldice_fwd leaves in UNet.cldice_sums (rsu_cldice.h). Plain arithmetic: floats, numpy
    arrays and tensors alike; empty sums give clD = 1."""
    Tp, Ts = (A + smooth) / (Bp + smooth), (Cc + smooth) / (Dy + smooth)
    return 2.0 * Tp * Ts / (Tp + Ts)


def parse_dice_smooth(value):
    """The --dice_smooth value as a float: finite and > 0. Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError("--dice_smooth must be a finite float > 0, not %r" % (value,))
    return v


def parse_border_weight(value):
    """The --border_weight value as a float: finite and >= 0 (0.0 = no border map). Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError("--border_weight must be a finite float >= 0, not %r" % (value,))
    return v


def parse_border_sigma(value):
    """The --border_sigma value as a float: finite and > 0. Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError("--border_sigma must be a finite float > 0, not %r" % (value,))
    return v


def parse_clip_grad_norm(value):
    """The --clip_grad_norm value as a float: 0 (off) or finite and > 0. Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (math.isfinite(v) and v >= 0.0):
        raise ValueError("--clip_grad_norm must be 0 (off) or a finite float > 0, not %r" % (value,))
    return v


def parse_ema_decay(value):
    """The --ema_decay value as a float: 0 (off) or in (0, 1). Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (0.0 <= v and np.float32(v) < np.float32(1.0)):
        raise ValueError("--ema_decay must be 0 (off) or a float in (0, 1), not %r" % (value,))
    return v


def parse_weight_decay(value):
    """The --weight_decay value as a float: 0 (off) or finite and > 0. Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (math.isfinite(v) and v >= 0.0):
        raise ValueError("--weight_decay must be 0 (off) or a finite float > 0, not %r" % (value,))
    return v


def parse_weight_decay_mode(value):
    """The --weight_decay_mode value: "decoupled" or "l2". Anything else raises ValueError."""
    if value not in DECAY_MODES:
        raise ValueError("--weight_decay_mode must be one of %s, not %r" % ("|".join(DECAY_MODES), value))
    return value


def parse_lr_schedule(value):
    """The --lr_schedule value: one of unet.LR_SCHEDULES. Anything else raises ValueError."""
    if value not in LR_SCHEDULES:
        raise ValueError("--lr_schedule must be one of %s, not %r" % ("|".join(LR_SCHEDULES), value))
    return value


def parse_lr_steps(value, flag):
    """The --lr_warmup_steps / --lr_total_steps value as an int >= 0. Anything else raises ValueError."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
        raise ValueError("--%s must be an integer >= 0, not %r" % (flag, value))
    return int(value)


def parse_lr_final(value):
    """The --lr_final value as a float in [0, 1]. Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (0.0 <= v <= 1.0):
        raise ValueError("--lr_final must be a float in [0, 1], not %r" % (value,))
    return v


def steps_per_epoch(num_patches, batch_size):
    """Optimizer steps of one train() call over num_patches patches: the length of the reference's `range(0, N - batch_size, batch_size)`
    (the final batch is dropped even when full). batch_size is the effective global batch of one step, so neither the number of GPUs
    nor --accumulate_steps changes the count."""
    return len(range(0, int(num_patches) - int(batch_size), int(batch_size)))


def parse_random_rotation(value):
    """The --random_rotation value as a float of degrees: finite and >= 0 (0.0 = off). Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (math.isfinite(v) and v >= 0.0):
        raise ValueError("--random_rotation must be a finite number of degrees >= 0, not %r" % (value,))
    return v


def parse_random_scale(value):
    """The --random_scale value: "LO,HI" or a pair of numbers -> (lo, hi) as floats with 1/64 < lo <= hi <= 64 ((1.0, 1.0) = off).
    Anything else raises ValueError."""
    if isinstance(value, str):
        parts = value.split(",")
    else:
        try:
            parts = list(value)
        except TypeError:
            parts = [value]
    try:
        sc = tuple(float(v) for v in parts)
    except (TypeError, ValueError):
        sc = ()
    if len(sc) != 2 or not all(math.isfinite(v) for v in sc) or not (1.0 / 64 < sc[0] <= sc[1] <= 64.0):
        raise ValueError("--random_scale must be 'LO,HI' with 1/64 < LO <= HI <= 64, not %r" % (value,))
    return sc


def parse_color_jitter(value):
    """The --color_jitter value: "B,C,S,H" or four numbers -> (B, C, S, H) as floats with B, C, S finite in [0, 1) and H in [0, 180]
    ((0.0, 0.0, 0.0, 0.0) = off). Anything else raises ValueError."""
    if isinstance(value, str):
        parts = value.split(",")
    else:
        try:
            parts = list(value)
        except TypeError:
            parts = [value]
    try:
        cj = () if any(isinstance(v, bool) for v in parts) else tuple(float(v) for v in parts)
    except (TypeError, ValueError):
        cj = ()
    if len(cj) != 4 or not all(math.isfinite(v) for v in cj) or not all(0.0 <= v < 1.0 for v in cj[:3]) or not 0.0 <= cj[3] <= 180.0:
        raise ValueError("--color_jitter must be 'B,C,S,H' with B, C, S in [0, 1) and H in [0, 180] degrees, not %r" % (value,))
    return cj


def parse_random_noise(value):
    """The --random_noise value as a float in [0, 1] (0.0 = off). Anything else raises ValueError."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (math.isfinite(v) and 0.0 <= v <= 1.0):
        raise ValueError("--random_noise must be a float in [0, 1], not %r" % (value,))
    return v


def parse_elastic_deformation(value):
    """The --elastic_deformation value: "ALPHA,GRID" or a pair -> (alpha, grid) as (float, int) with alpha finite in [0, 64] (0.0 = off) and
    grid an integer in [1, 16]. Anything else raises ValueError."""
    if isinstance(value, str):
        parts = value.split(",")
    else:
        try:
            parts = list(value)
        except TypeError:
            parts = [value]
    try:
        if len(parts) != 2 or any(isinstance(v, bool) for v in parts):
            raise ValueError
        alpha = float(parts[0])
        grid = int(parts[1].strip()) if isinstance(parts[1], str) else parts[1]   # ("3.0" and 3.5 are not integers)
        if not isinstance(grid, (int, np.integer)) or not (math.isfinite(alpha) and 0.0 <= alpha <= 64.0) or not 1 <= grid <= 16:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("--elastic_deformation must be 'ALPHA,GRID' with ALPHA in [0, 64] pixels and an integer GRID in [1, 16], not %r"
                         % (value,)) from None
    return alpha, int(grid)


def parse_accumulate_steps(value):
    """The --accumulate_steps value as an int >= 1 (1 = off). Anything else raises ValueError."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError("--accumulate_steps must be an integer >= 1, not %r" % (value,))
    return int(value)


def micro_batch_size(batch_size, world, accumulate_steps):
    """Patches per GPU and backward pass: batch_size / (world x accumulate_steps), which must divide (ValueError otherwise)."""
    if batch_size < 1 or batch_size % (world * accumulate_steps) != 0:
        raise ValueError("--batch_size=%d must be a positive multiple of %d GPU(s) x --accumulate_steps=%d: it is the effective batch "
                         "of one optimizer step" % (batch_size, world, accumulate_steps))
    return batch_size // (world * accumulate_steps)


def dice_from_sums(I, P, Y, smooth):
    """Soft Dice D = (2 I + s) / (P + Y + s) from the sums I = sum m p y, P = sum m p, Y = sum m y that the head leaves in UNet.dice_sums
    (rsu.h rsu_head_dice_sums). Plain arithmetic: floats, numpy arrays and tensors alike; empty sums give D = 1."""
    return (2.0 * I + smooth) / (P + Y + smooth)


def metrics_from_eval(sums, hist, n_pixels, dice_weight=0.0, dice_smooth=1.0, threshold=0.5):
    """What a validation pass reports, from the accumulators of rsu.h rsu_head_eval read back once (numpy and python floats only).
    sums = {sum omega CE, sum omega, I, P, Y}; hist [2][256]: per label, the count of pixels whose probability fell into bin
    min(255, int(p * 256)); n_pixels: the number of real pixels evaluated (padding excluded, ignored pixels included), the training
    loss's divisor. Returns a dict:
      loss = sums[0] / n_pixels; weighted_mean_loss = sums[0] / sums[1] (0 where sums[1] is 0); dice = dice_from_sums(I, P, Y, dice_smooth)
      (1 for an empty set); objective = loss + dice_weight * (1 - dice): the training objective over the whole set;
      tp, fp, fn, tn at `threshold`, which must be a multiple of 1/256 in [0, 1] (ValueError otherwise): a pixel is predicted road iff its
      bin >= round(threshold * 256), i.e. iff p >= threshold, exactly; accuracy, precision, recall, f1 with summary.StreamingMetrics.values'
      conventions (0 where a denominator is 0; f1 = 0 where recall or precision is), iou = tp / (tp + fp + fn) (0 where empty);
      best_threshold, best_f1 over the 255 interior thresholds k / 256, the lowest threshold winning ties; n_pixels, n_counted."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1)
    hist = np.asarray(hist)
    nbins = hist.shape[-1] if hist.ndim == 2 else 0
    if sums.size != 5 or hist.ndim != 2 or hist.shape[0] != 2 or nbins < 2:
        raise ValueError("metrics_from_eval needs sums of 5 values and a histogram [2][bins], not %s and %s" % (sums.shape, hist.shape))
    hist = hist.astype(np.int64)
    threshold = float(threshold)
    k = int(round(threshold * nbins)) if math.isfinite(threshold) else -1
    if not (0 <= k <= nbins) or k != threshold * nbins:
        raise ValueError("threshold must be a multiple of 1/%d in [0, 1], not %r: the counts come from a %d-bin histogram" % (nbins, threshold, nbins))
    n_pixels = int(n_pixels)
    loss = float(sums[0]) / n_pixels if n_pixels > 0 else 0.0
    dice = float(dice_from_sums(float(sums[2]), float(sums[3]), float(sums[4]), float(dice_smooth)))

    def scores(tp, fp, fn, tn):
        total = tp + fp + fn + tn
        accuracy = (tp + tn) / total if total else 0.0
        recall = tp / (tp + fn) if tp + fn else 0.0
        precision = tp / (tp + fp) if tp + fp else 0.0
        f1 = 0.0 if recall == 0.0 or precision == 0.0 else 2.0 / (1.0 / recall + 1.0 / precision)
        iou = tp / (tp + fp + fn) if tp + fp + fn else 0.0
        return accuracy, precision, recall, f1, iou

    # above[l][k] = pixels of label l in bins >= k, for k = 0 .. nbins
    above = np.concatenate([np.cumsum(hist[:, ::-1], axis=1)[:, ::-1], np.zeros((2, 1), np.int64)], axis=1)
    n0, n1 = int(hist[0].sum()), int(hist[1].sum())

    def counts(kk):
        tp, fp = int(above[1, kk]), int(above[0, kk])
        return float(tp), float(fp), float(n1 - tp), float(n0 - fp)

    tp, fp, fn, tn = counts(k)
    accuracy, precision, recall, f1, iou = scores(tp, fp, fn, tn)
    best_k, best_f1 = 1, -1.0
    for kk in range(1, nbins):
        f = scores(*counts(kk))[3]
        if f > best_f1:
            best_k, best_f1 = kk, f
    return {"loss": loss, "weighted_mean_loss": float(sums[0]) / float(sums[1]) if sums[1] != 0 else 0.0, "dice": dice,
            "objective": loss + float(dice_weight) * (1.0 - dice), "threshold": threshold,
            "tp": int(tp), "fp": int(fp), "fn": int(fn), "tn": int(tn),
            "accuracy": accuracy, "precision": precision, "recall": recall, "f1": f1, "iou": iou,
            "best_threshold": best_k / float(nbins), "best_f1": best_f1, "n_pixels": n_pixels, "n_counted": n0 + n1}


def balanced_class_weights(groundtruth):
    """(N / (2 N_0), N / (2 N_1)) over the labels of `groundtruth` binarised at 0.5 (tf_aerial_images.py:220), scikit-learn's "balanced"
    rule: each class carries half of the total weight and the mean weight over the data is 1, so the loss scale and a tuned --lr
    stay comparable with the unweighted loss. A class without pixels raises ValueError."""
    road = np.asarray(groundtruth) >= 0.5
    n, n1 = int(road.size), int(road.sum())
    n0 = n - n1
    if n0 == 0 or n1 == 0:
        raise ValueError("balanced class weights need both classes in the ground truth (background %d, road %d pixels)" % (n0, n1))
    return n / (2.0 * n0), n / (2.0 * n1)


class Options(object):
    """Options used by our model (tf_aerial_images.py:51-84). Construct with keyword overrides of the flag defaults;
    `rotation_angles` accepts the flag string "a,b,c" and is stored as a list of ints like the reference."""

    def __init__(self, **overrides):
        for name, _typ, default, _help in FLAG_DEFS + EXTRA_FLAG_DEFS:
            setattr(self, name, default)
        for k, v in overrides.items():
            if not hasattr(self, k):
                raise AttributeError("unknown option %r" % k)
            setattr(self, k, v)
        if self.optimizer not in ("momentum", "adam"):
            raise ValueError("--optimizer must be momentum or adam, not %r" % (self.optimizer,))
        self.class_weights = parse_class_weights(self.class_weights)   # None, (w0, w1) or "balanced" (cli.main resolves it)
        self.dice_weight, self.dice_smooth = parse_dice_weight(self.dice_weight), parse_dice_smooth(self.dice_smooth)
        self.focal_gamma = parse_focal_gamma(self.focal_gamma)
        self.cldice_weight, self.cldice_iters = parse_cldice_weight(self.cldice_weight), parse_cldice_iters(self.cldice_iters)
        self.cldice_smooth = parse_cldice_smooth(self.cldice_smooth)
        self.lovasz_weight = parse_lovasz_weight(self.lovasz_weight)
        self.min_road_area = parse_component_area(self.min_road_area, "min_road_area")
        self.max_hole_area = parse_component_area(self.max_hole_area, "max_hole_area")
        self.component_connectivity = parse_component_connectivity(self.component_connectivity)
        self.validate_components = bool(self.validate_components)
        self.validate_distances = bool(self.validate_distances)
        self.relaxed_slack = parse_relaxed_slack(self.relaxed_slack)
        self.save_best_metric = parse_save_best_metric(self.save_best_metric)
        if self.save_best_metric == "relaxed_f1" and not self.validate_distances:
            raise ValueError("--save_best_metric=relaxed_f1 requires --validate_distances: without it validation measures no distances")
        self.validate_centerlines, self.save_centerlines = bool(self.validate_centerlines), bool(self.save_centerlines)
        self.centerline_max_iters = parse_centerline_max_iters(self.centerline_max_iters)
        if self.save_best_metric == "cl_quality" and not self.validate_centerlines:
            raise ValueError("--save_best_metric=cl_quality requires --validate_centerlines: without it validation extracts no centre-lines")
        self.centerline_min_branch = parse_centerline_min_branch(self.centerline_min_branch)
        self.validate_junctions = bool(self.validate_junctions)
        if self.validate_junctions and not self.validate_centerlines:
            raise ValueError("--validate_junctions requires --validate_centerlines: without it validation extracts no centre-lines")
        self.validate_segments, self.save_road_graph = bool(self.validate_segments), bool(self.save_road_graph)
        self.max_segments = parse_max_segments(self.max_segments)
        self.road_graph_paths = bool(self.road_graph_paths)
        self.max_path_length = parse_max_path_length(self.max_path_length)
        self.road_graph_simplify = parse_road_graph_simplify(self.road_graph_simplify)
        if self.validate_segments and not self.validate_centerlines:
            raise ValueError("--validate_segments requires --validate_centerlines: without it validation extracts no centre-lines")
        self.validate_routes, self.road_graph_distances = bool(self.validate_routes), bool(self.road_graph_distances)
        self.max_graph_nodes, self.route_snap = parse_max_graph_nodes(self.max_graph_nodes), parse_route_snap(self.route_snap)
        if self.validate_routes and not self.validate_segments:
            raise ValueError("--validate_routes requires --validate_segments: without it validation extracts no road segments")
        if self.save_best_metric == "apls" and not self.validate_routes:
            raise ValueError("--save_best_metric=apls requires --validate_routes: without it validation measures no path lengths")
        self.border_weight, self.border_sigma = parse_border_weight(self.border_weight), parse_border_sigma(self.border_sigma)
        self.clip_grad_norm = parse_clip_grad_norm(self.clip_grad_norm)
        self.ema_decay, self.ema_warmup = parse_ema_decay(self.ema_decay), bool(self.ema_warmup)
        for name in ("validation_images", "validate_every"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError("--%s must be an integer >= 0, not %r" % (name, v))
            setattr(self, name, int(v))
        self.save_best = bool(self.save_best)
        self.random_rotation, self.random_scale = parse_random_rotation(self.random_rotation), parse_random_scale(self.random_scale)
        self.one_launch_loader = bool(self.one_launch_loader)
        self.color_jitter, self.random_noise = parse_color_jitter(self.color_jitter), parse_random_noise(self.random_noise)
        self.elastic_deformation = parse_elastic_deformation(self.elastic_deformation)
        self.accumulate_steps = parse_accumulate_steps(self.accumulate_steps)
        if self.accumulate_steps > 1:   # (the number of GPUs is known where the model is built: it checks again with it)
            micro_batch_size(self.batch_size, 1, self.accumulate_steps)
        self.weight_decay, self.weight_decay_mode = parse_weight_decay(self.weight_decay), parse_weight_decay_mode(self.weight_decay_mode)
        self.lr_schedule, self.lr_final = parse_lr_schedule(self.lr_schedule), parse_lr_final(self.lr_final)
        self.lr_warmup_steps = parse_lr_steps(self.lr_warmup_steps, "lr_warmup_steps")
        self.lr_total_steps = parse_lr_steps(self.lr_total_steps, "lr_total_steps")   # (0 with cosine | linear: resolved by cli.main)
        loader_flags = [name for name, on in (("--random_rotation", self.random_rotation > 0.0), ("--random_scale", self.random_scale != (1.0, 1.0)),
                                              ("--one_launch_loader", self.one_launch_loader),
                                              ("--color_jitter", any(v > 0.0 for v in self.color_jitter)),
                                              ("--random_noise", self.random_noise > 0.0),
                                              ("--elastic_deformation", self.elastic_deformation[0] > 0.0)) if on]
        if loader_flags and not self.device_patch_pool:   # (not silently ignored, the way --d4_augmentation is there)
            raise ValueError("%s cannot be combined with --nodevice_patch_pool: the kernels that apply them work on the batches of the device "
                             "patch pool; the host pool cuts plain windows only" % ", ".join(loader_flags))
        ra = self.rotation_angles
        if isinstance(ra, str):
            self.rotation_angles = None if not ra else [int(i) for i in ra.split(",")]


def pixel_f1(pred_masks, true_masks, threshold=0.5):
    """F1 = 2 / (1/recall + 1/precision) (summary.py:141-147) at pixel level on binarised masks."""
    p = np.asarray(pred_masks).reshape(-1) > threshold
    t = np.asarray(true_masks).reshape(-1) >= 0.5
    tp = float(np.logical_and(p, t).sum())
    if tp == 0:
        return 0.0
    recall, precision = tp / t.sum(), tp / p.sum()
    return 2.0 / (1.0 / recall + 1.0 / precision)


class ConvolutionalModel:
    def __init__(self, options, session=None, device=None, params=None):
        self._options = opts = options
        self._session = session  # kept for signature parity; unused
        np.random.seed(opts.seed)
        self.input_size = input_size_needed(opts.patch_size, opts.num_layers)
        self.experiment_name = datetime.now().strftime("%Y-%m-%dT%Hh%Mm%Ss")
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        assert opts.batch_size % self.world == 0, "global batch_size must divide evenly over ranks"
        # --accumulate_steps=K: one optimizer step over K passes per GPU; local_batch is the micro-batch, the batch of one pass
        self.accumulate_steps = K = int(getattr(opts, "accumulate_steps", 1))
        self.local_batch = micro_batch_size(opts.batch_size, self.world, K) if K > 1 else opts.batch_size // self.world
        if device is None:
            device = "cuda:%d" % (opts.gpu if opts.gpu >= 0 else int(os.environ.get("LOCAL_RANK", "0")))
        if torch.device(device).type == "cuda":
            torch.cuda.set_device(torch.device(device))  # the library works on the HIP current device (rsu.h "devices")
        # the reference's graph is static in (batch, patch): one UNet serves training and (zero-padded) prediction batches
        if opts.class_weights == "balanced":
            raise ValueError("class_weights='balanced' must be resolved from the training ground truth before the model is built: "
                             "options.class_weights = balanced_class_weights(groundtruth) (cli.main does)")
        self.net = UNet(opts.num_layers, opts.root_size, opts.dilated_layers, self.local_batch, opts.patch_size, device=device,
                        params=params, seed=opts.seed, training=True, optimizer=opts.optimizer, class_weights=opts.class_weights,
                        dice_weight=opts.dice_weight, dice_smooth=opts.dice_smooth, border_weight=opts.border_weight,
                        border_sigma=opts.border_sigma, clip_grad_norm=opts.clip_grad_norm if opts.clip_grad_norm > 0.0 else None,
                        ema_decay=opts.ema_decay if opts.ema_decay > 0.0 else None, ema_warmup=opts.ema_warmup,
                        accumulate_steps=K if K > 1 else None,
                        weight_decay=opts.weight_decay if getattr(opts, "weight_decay", 0.0) > 0.0 else None,
                        weight_decay_mode=getattr(opts, "weight_decay_mode", "decoupled"), focal_gamma=getattr(opts, "focal_gamma", 0.0),
                        cldice_weight=getattr(opts, "cldice_weight", 0.0), cldice_iters=getattr(opts, "cldice_iters", 10),
                        cldice_smooth=getattr(opts, "cldice_smooth", 1.0), lovasz_weight=getattr(opts, "lovasz_weight", 0.0))
        self.net.dropout_seed = int(opts.seed) + 7919 * self.rank  # independent masks on every rank's shard
        # --lr_schedule: cosine | linear with --lr_total_steps=0 wait for resolve_lr_total_steps() (the patches are not known yet)
        self._lr_unresolved = getattr(opts, "lr_schedule", "staircase") in ("cosine", "linear") and getattr(opts, "lr_total_steps", 0) < 1
        if not self._lr_unresolved:
            self._set_lr_schedule()
        self._bucketer = None
        self._exchange_tuned = False
        self.exchange_schedule = None
        self._uploader = None
        # summaries (tf_aerial_images.py:126-131,158-163): scalars loss + learning_rate per step, streaming train / eval scores
        # (created by the first train() call, so that prediction-only models leave no log directory behind)
        self._summary = None
        self._pending_scalars = []
        self.best_val_f1 = None   # the best validation F1 seen by train() (--save_best keeps that model)
        self.best_val_score = None   # the best validation --save_best_metric (the same figure unless it is relaxed_f1)
        self.last_postprocess_stats = None   # postprocess_masks: the summed stats of its last call (int64 [6])
        self._mask_metrics = None   # evaluate() with a --validate_* mask stage on: their one accumulator and device buffers (mask_metrics.py)
        if self.world > 1:
            self._bucketer = GradBucketer(self.net.flat_g, self.net.n_live)
            self._bucketer.extra_streams = list(self.net.wstreams)
            if K > 1:
                # a bucket launched during the last backward pass would send g_{K-1} without the local sum: on_grads stays unhooked,
                # the schedule is not tuned, and finish() all-reduces the whole buffer once, behind the K-th accumulate_gradients()
                self._exchange_tuned = True
            else:
                self.net.on_grads = self._bucketer.ready
            # identical initial weights on every rank (the reference has one copy; ranks must start from the same point)
            dist.broadcast(self.net.flat_w, 0)
            if self.net.flat_ema is not None:
                self.net.flat_ema.copy_(self.net.flat_w)   # (the shadows start at the broadcast weights)
            self.net.repack()

    # ------------------------------------------------------------------ training
    def _set_lr_schedule(self):
        opts = self._options
        self.net.set_lr_schedule(getattr(opts, "lr_schedule", "staircase"), getattr(opts, "lr_warmup_steps", 0), getattr(opts, "lr_total_steps", 0),
                                 getattr(opts, "lr_final", 0.0))

    def resolve_lr_total_steps(self, num_patches):
        """--lr_schedule=cosine|linear with --lr_total_steps=0: the horizon becomes this run's own length, --num_epoch times
        steps_per_epoch(num_patches, --batch_size), written back into the options and handed to the net; returns it. With any other
        combination of the two flags: nothing, returns --lr_total_steps as given. ValueError for a run that takes no step."""
        opts = self._options
        if not self._lr_unresolved:
            return opts.lr_total_steps
        total = int(opts.num_epoch) * steps_per_epoch(num_patches, opts.batch_size)
        if total < 1:
            raise ValueError("--lr_schedule=%s with --lr_total_steps=0 needs a run of at least one optimizer step: --num_epoch=%d over %d "
                             "patches at --batch_size=%d takes none" % (opts.lr_schedule, opts.num_epoch, num_patches, opts.batch_size))
        opts.lr_total_steps = total
        self._lr_unresolved = False
        self._set_lr_schedule()
        return total

    def train_step(self, patches, labels, weights=None):
        """One session.run([train, loss, predictions]) (tf_aerial_images.py:241-244) on this rank's shard.
        patches [b,S,S,3] float, labels [b,P,P] in {0,1}; returns (global mean loss tensor, predictions [b,P,P] device tensor).
        weights: an optional per-pixel weight map [b,P,P] for this step's loss (UNet.set_pixel_weights; it multiplies the model's
        class weights); None: no map, also after a step that had one. With class weights or a map the loss is the weighted sum over the
        GLOBAL pixel count (UNet.backward_device), and a label other than 0 and 1 then ignores its pixel: no loss, no gradient.
        With --dice_weight > 0 the returned loss is that cross-entropy + dice_weight * (1 - D), D the soft Dice of each rank's batch
        (averaged over the ranks), and labels other than 0 and 1 are ignored as well. --cldice_weight > 0 adds
        cldice_weight * (1 - clD) in the same way, clD the centre-line Dice of each rank's batch (rsu_cldice.h). --lovasz_weight > 0 adds
        lovasz_weight * the mean per-image Lovasz loss (rsu_lovasz.h) over every image of the step.
        With --accumulate_steps=K > 1 the three arrays hold the rank's whole share of the effective batch, [K*b, ...]: micro-batch j is
        rows [j*b, (j+1)*b), the step is ONE optimizer step, and the predictions come back as a new tensor [K*b,P,P].
        (Synchronous upload: the train() loop stages its batches one step ahead instead, see pool.BatchUploader.)"""
        net, K, b = self.net, self.accumulate_steps, self.local_batch
        x = torch.as_tensor(np.asarray(patches, dtype=np.float32))
        y = torch.as_tensor(np.asarray(labels))
        w = None if weights is None else torch.as_tensor(np.asarray(weights, dtype=np.float32))
        if K == 1:
            net.x.copy_(x.to(net.device))
            net.labels.copy_(y.to(net.device, torch.int64))
            net.set_pixel_weights(w)
            return self._run_step()
        if x.shape[0] != K * b or y.shape[0] != K * b or (w is not None and w.shape[0] != K * b):
            raise ValueError("train_step with --accumulate_steps=%d takes the rank's whole share: %d x %d patches, not %d" % (K, K, b, x.shape[0]))
        predictions = torch.empty((K * b,) + tuple(net.prob.shape[1:]), dtype=net.prob.dtype, device=net.device)

        def load(micro):
            sl = slice(micro * b, (micro + 1) * b)
            net.x.copy_(x[sl].to(net.device))
            net.labels.copy_(y[sl].to(net.device, torch.int64))
            net.set_pixel_weights(None if w is None else w[sl])

        def between(micro):
            predictions[micro * b:(micro + 1) * b].copy_(net.prob)

        loss, _ = self._run_step(load, between)
        between(K - 1)
        return loss, predictions

    def _run_step(self, load=None, between=None):
        """forward + loss + backward + gradient exchange + optimizer step (Momentum or Adam) on the batch held in net.x / net.labels.
        With --accumulate_steps=K > 1: K times load(micro) (which puts micro-batch `micro` there), forward, backward and
        net.accumulate_gradients(), the losses added up on the device, between(micro) behind every micro-batch but the last (whose
        labels and probabilities are still in the net when this returns, as they always were); then ONE exchange and ONE optimizer step."""
        opts, net, K = self._options, self.net, self.accumulate_steps
        if load is not None:
            load(0)   # (in front of the exchange tuning below, which times passes over the batch in the net)
        if self._bucketer is not None and not self._exchange_tuned:
            # first step of a data-parallel run: time forward + backward + exchange (no optimizer step, so the trajectory is
            # untouched) under both schedules and keep the faster one (dist.tune_overlap)
            self._exchange_tuned = True
            if "RSU_DP_OVERLAP" not in os.environ:
                def probe():
                    net.forward_device(keep=float(opts.dropout))
                    self._bucketer.reset()
                    net.backward_device(1.0 / (opts.batch_size * opts.patch_size * opts.patch_size))
                    self._bucketer.finish()
                def set_budget(n):   # every candidate budget gets its own (untimed) tile-shape tuning pass before it is timed
                    net.backward_cu_budget = n
                    net.ensure_tuned(keep=float(opts.dropout))
                self.exchange_schedule = tune_overlap(self._bucketer, probe, trials=2, set_cu_budget=set_budget)
        if self._bucketer is not None:
            self._bucketer.reset()   # (nothing is in flight between two steps: finish() has drained the last exchange)
        # the Dice term is each rank's own batch Dice -- with --accumulate_steps each micro-batch's -- scaled by 1 / (world * K): the SUM
        # all-reduce of the gradients and of the loss below, and the sum over the micro-batches, then give the mean over all of them,
        # with no collective inside the backward pass
        dice_scale = net.dice_weight / (self.world * K)
        cldice_scale = net.cldice_weight / (self.world * K)   # the clDice term likewise: each rank's, each micro-batch's own
        lovasz_scale = net.lovasz_weight / (self.world * K)   # a mean of per-image losses: with this the step's objective is one large batch's
        loss = None
        for micro in range(K):
            if load is not None and micro > 0:
                load(micro)
            net.ensure_tuned(keep=float(opts.dropout))   # the explicit tile-shape tuning pass (untimed, weights untouched): once, in front of the first step
            # feed_dict dropout_keep: opts.dropout (tf_aerial_images.py:237); the masks come from a counter-based hash of
            # (seed, rank, dropout site, global step, micro-batch, element) instead of TF's Philox stream
            net.forward_device(keep=float(opts.dropout))
            net.backward_device(1.0 / (opts.batch_size * opts.patch_size * opts.patch_size), dice_scale=dice_scale,
                                cldice_scale=cldice_scale, lovasz_scale=lovasz_scale)
            net.accumulate_gradients()   # (K == 1: nothing)
            part = net.loss_sum / (opts.batch_size * opts.patch_size * opts.patch_size)
            if dice_scale > 0.0:   # (device arithmetic on net.dice_sums: no synchronisation)
                s = net.dice_sums
                part = part + dice_scale * (1.0 - dice_from_sums(s[0:1], s[1:2], s[2:3], net.dice_smooth))
            if cldice_scale > 0.0:   # (likewise on net.cldice_sums)
                s = net.cldice_sums
                part = part + cldice_scale * (1.0 - cldice_from_sums(s[0:1], s[1:2], s[2:3], s[3:4], net.cldice_smooth))
            if lovasz_scale > 0.0:   # (likewise on net.lovasz_sum = {sum_b L_b, images})
                s = net.lovasz_sum
                part = part + lovasz_scale * s[0:1] / s[1:2]
            loss = part if loss is None else loss + part
            if between is not None and micro < K - 1:
                between(micro)
        if self._bucketer is not None:
            self._bucketer.finish()
            dist.all_reduce(loss)
        if opts.optimizer == "adam":
            net.apply_adam(opts.lr, opts.adam_beta1, opts.adam_beta2, opts.adam_epsilon)
        else:
            net.apply_momentum(opts.lr, opts.momentum)
        return loss, net.prob

    # ------------------------------------------------------------------ held-out validation
    def _averaged_ctx(self, averaged, what):
        """(context, averaged?) for the device work of evaluate() / predict(): net.averaged_weights() for averaged=True, or None on a net
        that has averages; the raw weights (a no-op context) for False, or None on a net without. True on a net without averages raises."""
        has = self.net.flat_ema is not None
        if averaged and not has:
            raise ValueError("%s(averaged=True) on a model without averaged weights (--ema_decay=0)" % what)
        use = has if averaged is None else bool(averaged)
        return (self.net.averaged_weights() if use else contextlib.nullcontext()), use

    @torch.no_grad()
    def evaluate(self, patches, labels, weights=None, threshold=0.5, averaged=None):
        """The training objective and the pixel metrics over a held-out set, forward only: `patches` [N,S,S,3] float, `labels` [N,P,P]
        (already 0 / 1; any other value ignores its pixel), `weights` an optional weight map [N,P,P] (None: no map). Every rank must call
        it with the same set. The set is sharded contiguously over the ranks and run in local_batch chunks -- the last one padded with
        zero patches whose labels are -1, which the head ignores: the padding adds exactly nothing -- through UNet.forward_device(keep=1)
        and UNet.evaluate_device (one rsu_head_eval launch per chunk). Everything accumulates on the device; the two accumulators are
        SUM-all-reduced (the sums as float64) and read back ONCE. Returns metrics_from_eval(...) of them, with the net's dice_weight /
        dice_smooth, plus "sums" (float64 [5]) and "hist" (int64 [2, 256]), and "cldice_sums" (float64 [4]: {A, Bp, Cc, Dy} over the set,
        all-reduced with the others; zeros with --cldice_weight=0) with "cldice" = cldice_from_sums of them; with --cldice_weight > 0
        "objective" also includes cldice_weight * (1 - cldice). With --lovasz_weight > 0 (only then) also "lovasz", the mean per-image
        Lovasz loss over the set from the all-reduced {sum_b L_b, images} less the padding images (which add exactly 0), and
        "objective" includes lovasz_weight * lovasz. With any of --validate_components, --validate_distances and --validate_centerlines
        (with it --centerline_min_branch, --validate_junctions, --validate_segments), and only then, the integer mask metrics of
        mask_metrics.MaskMetrics: its launches per chunk behind the head on net.prob and net.labels at `threshold`, its counters last in
        the same all-reduce and read-back (exact in float64 below 2^53), and the result gains the keys of mask_metrics.decode.
        averaged: None scores the averaged weights when the net has them (--ema_decay), True demands them (ValueError on a net without),
        False forces the raw weights; the device work runs inside net.averaged_weights(), and the result carries "averaged" (bool).
        Training is left as it was: weights, the averages and every packed copy (the exchange of averaged_weights() is undone), optimizer
        slots, global_step (and with it the dropout keys), the gradient buffers, net.x / net.labels, net.pixel_weights and a batch the
        uploader has staged; net.prob holds the last chunk's probabilities afterwards."""
        net, B = self.net, self.local_batch
        patches, labels = np.asarray(patches), np.asarray(labels)
        N = int(patches.shape[0])
        if labels.shape[0] != N or (weights is not None and len(weights) != N):
            raise ValueError("evaluate: %d patches, %d label tiles%s" % (N, labels.shape[0], "" if weights is None else ", %d weight maps" % len(weights)))
        metrics_from_eval(np.zeros(5), np.zeros((2, net.eval_hist.shape[1]), np.int64), 0, threshold=threshold)   # a bad threshold fails before any work
        per = -(-N // self.world)
        lo, hi = min(self.rank * per, N), min((self.rank + 1) * per, N)
        ctx, averaged = self._averaged_ctx(averaged, "evaluate")
        net.ensure_tuned(training=False, keep=1.0)   # (an untimed pass of its own kind; under data parallelism no collective is in flight here)
        x0, l0 = net.x.clone(), net.labels.clone()
        pw0 = net.pixel_weights.clone() if net.pixel_weights is not None else None
        try:
            with ctx:
                net.reset_eval()
                mm = self._ensure_mask_metrics()
                if mm is not None:
                    mm.reset()
                for t0 in range(lo, hi, B):
                    nb = min(B, hi - t0)
                    if nb < B:
                        net.x.zero_()
                        net.labels.fill_(-1)
                    net.x[:nb].copy_(torch.as_tensor(np.asarray(patches[t0:t0 + nb], dtype=np.float32)))
                    net.labels[:nb].copy_(torch.as_tensor(np.asarray(labels[t0:t0 + nb])).to(torch.int64))
                    if weights is not None:
                        wmap = np.ones((B,) + tuple(labels.shape[1:]), dtype=np.float32)
                        wmap[:nb] = np.asarray(weights[t0:t0 + nb], dtype=np.float32)
                        net.set_pixel_weights(torch.from_numpy(wmap))
                    else:
                        net.set_pixel_weights(None)
                    net.forward_device(keep=1.0)
                    net.evaluate_device()
                    if mm is not None:
                        mm.run(net.prob, net.labels, threshold)
                sums, hist = net.eval_sums.to(torch.float64), net.eval_hist.clone()
                with_cl = net.cldice_weight > 0.0
                if with_cl:   # the four clDice sums ride behind the five of the head: one all-reduce, one read-back
                    sums = torch.cat([sums, net.eval_cldice_sums.to(torch.float64)])
                with_lv = net.lovasz_weight > 0.0
                if with_lv:   # and the Lovasz pair {sum_b L_b, images} last
                    sums = torch.cat([sums, net.eval_lovasz_sum.to(torch.float64)])
                if mm is not None:   # and the mask stages' integer counters behind everything else
                    sums = torch.cat([sums, mm.acc.to(torch.float64)])
                if self.world > 1:
                    dist.all_reduce(sums)
                    dist.all_reduce(hist)
                sums, hist = sums.cpu().numpy(), hist.cpu().numpy()   # the one synchronisation
                if mm is not None:
                    sums, mask_counts = sums[:-mm.acc.numel()], sums[-mm.acc.numel():]
                lv_sums = sums[-2:] if with_lv else None
                sums, cl_sums = sums[:5], (sums[5:9] if with_cl else np.zeros(4))
        finally:
            net.x.copy_(x0)
            net.labels.copy_(l0)
            net.set_pixel_weights(pw0)
        out = metrics_from_eval(sums, hist, N * int(np.prod(labels.shape[1:])), net.dice_weight, net.dice_smooth, threshold)
        out["sums"], out["hist"], out["averaged"] = sums, hist, averaged
        out["cldice_sums"] = cl_sums
        out["cldice"] = float(cldice_from_sums(float(cl_sums[0]), float(cl_sums[1]), float(cl_sums[2]), float(cl_sums[3]), net.cldice_smooth))
        if with_cl:
            out["objective"] = out["objective"] + net.cldice_weight * (1.0 - out["cldice"])
        if with_lv:   # the mean over the set's N images: the chunks' padding images have no counted pixel, L_b = 0
            out["lovasz"] = float(lv_sums[0]) / max(N, 1)
            out["objective"] = out["objective"] + net.lovasz_weight * out["lovasz"]
        if mm is not None:
            out.update(mm.decode(mask_counts))
        return out

    def _ensure_mask_metrics(self):
        """the owner of the mask stages' device buffers (mask_metrics.MaskMetrics), made when evaluate() first needs it; None while no
        --validate_* flag of its stages is on: no call, no buffer, no key"""
        opts = self._options
        flags = mask_metrics.Flags.of(opts)
        if not flags.any:
            return None
        if self._mask_metrics is None or self._mask_metrics.flags != flags:
            self._mask_metrics = mask_metrics.MaskMetrics(
                flags, self.net.device, self.local_batch, self.net.P, connectivity=getattr(opts, "component_connectivity", 8),
                max_iters=getattr(opts, "centerline_max_iters", 64), max_segments=getattr(opts, "max_segments", 4096),
                relaxed_slack=getattr(opts, "relaxed_slack", 0), max_nodes=getattr(opts, "max_graph_nodes", 256),
                route_snap=getattr(opts, "route_snap", 8))
        return self._mask_metrics

    def _validate(self, validation, step):
        """one validation pass inside train(): evaluate (the averaged weights with --ema_decay), print and log on rank 0, keep the best model
        with --save_best (its checkpoint holds the raw weights and the averages)"""
        opts = self._options
        v = self.evaluate(validation[0], validation[1])
        if self.rank == 0:
            print("\nstep {} validation: loss {:.5f} objective {:.5f} dice {:.4f} f1 {:.4f} iou {:.4f} best threshold {:.4f} (f1 {:.4f}) on {} patches{}"
                  .format(step, v["loss"], v["objective"], v["dice"], v["f1"], v["iou"], v["best_threshold"], v["best_f1"], len(validation[0]),
                          " (averaged weights)" if v["averaged"] else ""))
            if "b0_error" in v:
                print("step {} validation components: predicted {} true {} b0_error {:.4f}".format(step, v["components_pred"],
                                                                                                 v["components_true"], v["b0_error"]))
            if "relaxed_f1" in v:
                print("step {} validation distances: relaxed f1 {:.4f} precision {:.4f} recall {:.4f} at slack {}; mean distance predicted "
                      "{:.3f} true {:.3f}; beyond 62 pixels: predicted {:.4f} true {:.4f}"
                      .format(step, v["relaxed_f1"], v["relaxed_precision"], v["relaxed_recall"], opts.relaxed_slack, v["mean_dist_pred"],
                              v["mean_dist_true"], v["far_pred"], v["far_true"]))
            if "cl_quality" in v:
                print("step {} validation centre-lines: quality {:.4f} completeness {:.4f} correctness {:.4f} at slack {}; hard clDice {:.4f}; "
                      "skeleton pixels predicted {} true {}; unconverged image sides {}"
                      .format(step, v["cl_quality"], v["cl_completeness"], v["cl_correctness"], opts.relaxed_slack, v["cldice_hard"],
                              v["cl_len_pred"], v["cl_len_true"], v["thin_unconverged"]))
            if "jn_f1" in v:
                print("step {} validation junctions: f1 {:.4f} precision {:.4f} recall {:.4f} at slack {}; junctions predicted {} true {} "
                      "error {:.4f}; ends predicted {} true {}; isolated pixels predicted {} true {}"
                      .format(step, v["jn_f1"], v["jn_precision"], v["jn_recall"], opts.relaxed_slack, v["junctions_pred"],
                              v["junctions_true"], v["junction_error"], v["ends_pred"], v["ends_true"], v["isolated_pred"],
                              v["isolated_true"]))
            if "length_ratio" in v:
                print("step {} validation road segments: predicted {} true {}; road length predicted {:.1f} true {:.1f} (ratio {:.4f}); "
                      "nodes predicted {} true {}; dangling predicted {} true {}; multi predicted {} true {}; dropped predicted {} true {}"
                      .format(step, v["segments_pred"], v["segments_true"], v["road_length_pred"], v["road_length_true"], v["length_ratio"],
                              v["nodes_pred"], v["nodes_true"], v["dangling_pred"], v["dangling_true"], v["multi_pred"], v["multi_true"],
                              v["segments_dropped_pred"], v["segments_dropped_true"]))
            if "apls" in v:
                print("step {} validation path lengths: APLS {:.4f} (truth to prediction {:.4f} over {} pairs, {} unmatched, {} broken; "
                      "prediction to truth {:.4f} over {} pairs, {} unmatched, {} broken); nodes predicted {} true {}, past --max_graph_nodes {} {}"
                      .format(step, v["apls"], v["apls_true_to_pred"], v["route_pairs_true_to_pred"], v["route_unmatched_true_to_pred"],
                              v["route_broken_true_to_pred"], v["apls_pred_to_true"], v["route_pairs_pred_to_true"],
                              v["route_unmatched_pred_to_true"], v["route_broken_pred_to_true"], v["graph_nodes_pred"], v["graph_nodes_true"],
                              v["graph_nodes_dropped_pred"], v["graph_nodes_dropped_true"]))
            if self._summary is not None:
                self._summary.add({"val_loss": v["loss"], "val_objective": v["objective"], "val_dice": v["dice"], "val_f1": v["f1"],
                                   "val_iou": v["iou"], "val_best_threshold": v["best_threshold"]}, global_step=step)
                if opts.cldice_weight > 0.0:
                    self._summary.add({"val_cldice": v["cldice"]}, global_step=step)
                if opts.lovasz_weight > 0.0:
                    self._summary.add({"val_lovasz": v["lovasz"]}, global_step=step)
                if "b0_error" in v:
                    self._summary.add({"val_b0_error": v["b0_error"]}, global_step=step)
                if "relaxed_f1" in v:
                    self._summary.add({"val_relaxed_f1": v["relaxed_f1"], "val_relaxed_precision": v["relaxed_precision"],
                                       "val_relaxed_recall": v["relaxed_recall"], "val_mean_dist_pred": v["mean_dist_pred"],
                                       "val_mean_dist_true": v["mean_dist_true"]}, global_step=step)
                if "cl_quality" in v:
                    self._summary.add({"val_cl_quality": v["cl_quality"], "val_cl_completeness": v["cl_completeness"],
                                       "val_cl_correctness": v["cl_correctness"], "val_cldice_hard": v["cldice_hard"]}, global_step=step)
                if "jn_f1" in v:
                    self._summary.add({"val_jn_f1": v["jn_f1"], "val_jn_precision": v["jn_precision"], "val_jn_recall": v["jn_recall"],
                                       "val_junction_error": v["junction_error"]}, global_step=step)
                if "length_ratio" in v:
                    self._summary.add({"val_length_ratio": v["length_ratio"], "val_road_length_pred": v["road_length_pred"],
                                       "val_road_length_true": v["road_length_true"]}, global_step=step)
                if "apls" in v:
                    self._summary.add({"val_apls": v["apls"], "val_apls_true_to_pred": v["apls_true_to_pred"],
                                       "val_apls_pred_to_true": v["apls_pred_to_true"]}, global_step=step)
        # (the same numbers on every rank: they come out of the all-reduce)
        if self.best_val_f1 is None or v["f1"] > self.best_val_f1:
            self.best_val_f1 = v["f1"]
        score = v[getattr(opts, "save_best_metric", "f1")]   # what --save_best compares: with the default v["f1"], and best_val_score is best_val_f1
        if self.best_val_score is None or score > self.best_val_score:
            self.best_val_score = score
            if opts.save_best:
                self.save_as(os.path.abspath(os.path.join(opts.save_path, self.experiment_name + "-best.chkpt")))
        return {k: v[k] for k in v if k not in ("sums", "hist", "cldice_sums", "dist_hist", "cl_hist", "jn_hist")}

    def _ensure_summary(self):
        opts = self._options
        if self._summary is None and self.rank == 0 and getattr(opts, "logdir", None):
            self._summary = Summary(opts, self._session, os.path.join(opts.logdir, self.experiment_name), device=self.net.device)
            self._summary.initialize_eval_summary()
            self._summary.initialize_train_summary()
            self._summary.initialize_overlap_summary()
            self._summary.initialize_missclassification_summary()
            tags = {"loss": None, "learning_rate": None}
            if self.net.clip_state is not None:
                tags["grad_norm"] = None
            self.summary_op = self._summary.get_summary_op(tags)
        return self._summary

    def _flush_scalars(self):
        """the per-step scalars are kept as device tensors and written in batches: reading them back every step would serialise
        the host with the GPU (the reference's session.run does exactly that)"""
        if self._summary is not None:
            for step, loss_t, err_t, total, lr, norm_t in self._pending_scalars:
                self._summary.add({"loss": float(loss_t), "learning_rate": lr}, global_step=step)
                if norm_t is not None:   # --clip_grad_norm: the norm of the step's gradient, before clipping
                    self._summary.add({"grad_norm": float(norm_t)}, global_step=step)
                self._summary.add_to_pixel_missclassification_summary(float(err_t), total, step)
        self._pending_scalars = []

    def train(self, patches, labels_patches, imgs, labels, validation=None):
        """Train the model for one epoch (tf_aerial_images.py:212-269): binarise labels at 0.5, shuffle with np.random,
        `for offset in range(0, N - batch_size, batch_size)` (the final batch is dropped even when full).
        `patches` is the reference's [N,S,S,3] array (then `labels_patches` its [N,P,P] labels) or a pool.PatchPool /
        pool.DevicePatchPool holding the same patches as an index (then `labels_patches` is ignored).
        validation: None (the default: the epoch issues exactly the launches it always did) or a held-out (patches [n,S,S,3], labels
        [n,P,P] in {0,1}) pair (hostio.validation_patches): evaluate() runs on it every --validate_every steps, or once at the end of the
        epoch with --validate_every=0; rank 0 prints one line and logs val_loss, val_objective, val_dice, val_f1, val_iou and
        val_best_threshold; last_epoch_stats gains "validation" (the last pass's metrics); --save_best keeps the best model by val_f1."""
        opts, net = self._options, self.net
        if self._lr_unresolved:
            raise ValueError("--lr_schedule=%s with --lr_total_steps=0: call resolve_lr_total_steps(number of patches) before train() "
                             "(cli.main does)" % opts.lr_schedule)
        val_stats = None
        self._ensure_summary()
        pool = patches if isinstance(patches, PatchPool) else None
        if pool is None:
            labels_patches = (np.asarray(labels_patches) >= 0.5) * 1.
        if labels is not None:
            labels = (np.asarray(labels) >= 0.5) * 1.
        num_train_patches = patches.shape[0]
        indices = np.arange(0, num_train_patches)
        np.random.shuffle(indices)
        num_errors = torch.zeros((), dtype=torch.float64, device=net.device)
        total = 0
        last = None
        offsets = list(range(0, num_train_patches - opts.batch_size, opts.batch_size))
        device_pool = isinstance(pool, DevicePatchPool)
        if not device_pool and self._uploader is None and net.device.type == "cuda":
            self._uploader = BatchUploader(net)

        K = self.accumulate_steps   # micro-batches per optimizer step (--accumulate_steps; 1: the rank's share is one batch, as ever)

        def batch_indices(offset, micro):
            return micro_indices(indices, offset, opts.batch_size, self.rank, self.world, micro, K)   # (K == 1: shard_indices)

        def host_batch(offset, micro=0):
            idx = batch_indices(offset, micro)
            return pool.gather(idx) if pool is not None else (patches[idx], labels_patches[idx])

        if offsets and not device_pool:
            self._uploader.stage(0, *host_batch(offsets[0]))
        for batch_i, offset in enumerate(offsets):
            # the uploader's slot is the running (micro-)batch counter & 1: every batch is staged one ahead of the pass that reads it
            def load(micro, offset=offset, count=batch_i * K):
                if device_pool:
                    pool.load_batch(batch_indices(offset, micro), net.x, net.labels)
                else:
                    self._uploader.commit((count + micro) & 1)

            def between(micro, offset=offset, count=batch_i * K):   # behind every micro-batch but the step's last: never with K == 1
                if not device_pool:
                    self._uploader.stage((count + micro + 1) & 1, *host_batch(offset, micro + 1))  # rides beside the pass just launched
                num_errors.add_((net.labels.to(torch.float64) - net.prob.to(torch.float64)).abs().sum())

            loss, predictions = self._run_step(load, between)
            if not device_pool and batch_i + 1 < len(offsets):
                self._uploader.stage(((batch_i + 1) * K) & 1, *host_batch(offsets[batch_i + 1]))  # rides beside the step just launched
            step = net.global_step
            if self.rank == 0:
                print("Batch {} Step {}".format(batch_i, step), end="\r")
            num_errors += (net.labels.to(torch.float64) - predictions.to(torch.float64)).abs().sum()  # soft error (:249)
            total += opts.batch_size
            last = loss
            if self._summary is not None:
                # (with --clip_grad_norm also a clone of the norm in the device-resident state record: device work, no synchronisation)
                norm = net.clip_state.view(torch.float32)[1].clone() if net.clip_state is not None else None
                self._pending_scalars.append((step, loss.clone(), num_errors.clone(), total, net.learning_rate(opts.lr), norm))
                if len(self._pending_scalars) >= 64:
                    self._flush_scalars()
            # from time to time do full prediction on some images (tf_aerial_images.py:253-264)
            if step > 0 and step % opts.eval_every == 0 and imgs is not None:
                images_to_predict = np.asarray(imgs)[:opts.num_eval_images]
                masks = self.predict(images_to_predict)
                if self.rank == 0:
                    f1 = pixel_f1(masks, labels[:opts.num_eval_images])
                    print("\nstep {} loss {:.5f} pixel-F1 on {} eval images {:.4f}".format(step, float(loss), opts.num_eval_images, f1))
                    if self._summary is not None:
                        overlays = hostio.overlays(images_to_predict, masks)
                        pred_masks = ((masks > 0.5) * 1).squeeze(-1)
                        self._summary.add_to_eval_summary(masks, overlays, labels, step)
                        self._summary.add_to_overlap_summary(labels[:opts.num_eval_images], pred_masks, step)
            if step > 0 and step % opts.train_score_every == 0 and imgs is not None:
                train_masks = self.predict(np.asarray(imgs))  # tf_aerial_images.py:266-267
                if self._summary is not None:
                    self._summary.add_to_training_summary(train_masks, labels, step)
            if validation is not None and opts.validate_every > 0 and step > 0 and step % opts.validate_every == 0:
                val_stats = self._validate(validation, step)
        if validation is not None and opts.validate_every == 0:
            val_stats = self._validate(validation, net.global_step)
        if self._summary is not None:
            self._flush_scalars()
            self._summary.flush()
        self.last_epoch_stats = {"loss": None if last is None else float(last), "soft_errors": float(num_errors), "patches": total}
        if val_stats is not None:
            self.last_epoch_stats["validation"] = val_stats
        if net.clip_state is not None:   # --clip_grad_norm: steps / clipped / skipped so far, norm and scale of the last step
            self.last_epoch_stats["clip"] = net.clip_stats()
        return self.last_epoch_stats

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def predict(self, imgs, averaged=None):
        """Run inference on `imgs` and return predicted masks (tf_aerial_images.py:271-328).
        averaged: None predicts with the averaged weights when the net has them (--ema_decay), True demands them (ValueError on a net
        without), False forces the raw weights (evaluate has the same argument); the forward passes run inside net.averaged_weights().
        imgs: [num_images, H, W, 3] in [0,1], one shape per call, H and W at least --patch_size (ValueError otherwise) and any --stride:
        where the stride does not cover an axis its last tile is clamped to the image's edge (hostio.tile_origins). Returns numpy
        [num_images, H, W, 1] road probabilities.
        Ensemble x6 -> mirror border -> tiles (x-outer order) -> batched forward -> overlap average -> inverse ensemble. With H != W the
        quarter turns are W x H images: they are predicted in a pass of their own and the six terms added in the reference's order.
        Tiles are sharded contiguously over ranks; the accumulators are summed with one all-reduce."""
        opts, net = self._options, self.net
        ctx, _ = self._averaged_ctx(averaged, "predict")
        imgs_t = torch.as_tensor(np.asarray(imgs)).to(net.device, torch.float32)
        if imgs_t.dim() != 4 or imgs_t.shape[3] != 3:
            raise ValueError("predict: images must be [n, H, W, 3], not %s" % (tuple(imgs_t.shape),))
        H, W = int(imgs_t.shape[1]), int(imgs_t.shape[2])
        if H < opts.patch_size or W < opts.patch_size:
            raise ValueError("predict: an image of %d x %d pixels is smaller than --patch_size=%d: predict with a smaller --patch_size "
                             "(the weights do not depend on it)" % (H, W, opts.patch_size))
        was_training = net.training
        net.training = False
        try:
            with ctx:
                if not opts.ensemble_prediction:
                    masks = self._predict_masks(imgs_t)
                elif H == W:
                    masks = dimages.invert_image_augmentation_ensemble(self._predict_masks(dimages.image_augmentation_ensemble(imgs_t).contiguous()))
                else:
                    upright, turned = dimages.image_augmentation_ensemble_rect(imgs_t)
                    masks = dimages.invert_image_augmentation_ensemble_rect(self._predict_masks(upright.contiguous()),
                                                                            self._predict_masks(turned.contiguous()))
        finally:
            net.training = was_training
        return masks.cpu().numpy()

    def _predict_masks(self, imgs_t):
        """predict() behind the ensemble, for device images [n, H, W, 3] of one shape: the device masks [n, H, W, 1]. Runs inside predict's
        weight context with net.training off."""
        opts, net = self._options, self.net
        dev = net.device
        num_images, H, W = imgs_t.shape[0], imgs_t.shape[1], imgs_t.shape[2]
        P, S, B = opts.patch_size, self.input_size, self.local_batch
        acc = dimages.OverlapAccumulator(num_images, (H, W), P, opts.stride, device=dev)
        num_patches = num_images * acc.nx * acc.ny
        if os.environ.get("RSU_PREDICT_SHARED", "1") == "1" and acc.nx * acc.ny > 1:
            # every rank fills the tiles of its own phase classes (zeros elsewhere) and overlap-adds the lot locally: the hit counts are
            # then complete on every rank, and ONE all-reduce of the accumulator (H*W floats per image variant, 1.4 MB at 604 px --
            # not the 1.3 GB of tiles) completes the sums
            tiles = self._shared_window_tiles(imgs_t)
            acc.add(tiles.view(-1, P, P), 0)
            if self.world > 1:
                dist.all_reduce(acc.acc)
        else:
            per = -(-num_patches // self.world)
            lo, hi = min(self.rank * per, num_patches), min((self.rank + 1) * per, num_patches)
            net.ensure_tuned(training=False)
            for t0 in range(lo, hi, B):
                nb = min(B, hi - t0)
                if nb < B:
                    net.x.zero_()  # the reference pads the last batch with zero patches (tf_aerial_images.py:298-301)
                dimages.extract_mirrored_patches(imgs_t, S, P, opts.stride, t0=t0, ntiles=nb, out=net.x[:nb])
                net.forward_device()
                acc.add(net.prob[:nb], t0)
            if self.world > 1:
                dist.all_reduce(acc.acc)
                dist.all_reduce(acc.hits)
        return acc.finish()

    def _shared_window_tiles(self, imgs_t, pps=None):
        """The sliding window of tf_aerial_images.py:288-320 without its redundancy. The network is fully convolutional with VALID
        convolutions; its L-1 pools tie the result to the input offset modulo 2^(L-1) only. Tiles whose offsets agree modulo that
        period (on both axes) are therefore sub-windows of ONE forward pass over the union of their input windows: with stride 12
        and L = 6 the 19 x 19 tiles of a 604-pixel image fall into 8 x 8 phase classes of up to 3 x 3 tiles spaced lcm(12, 32) = 96
        pixels apart -- 64 passes over <= 956-pixel windows instead of 361 passes over 764-pixel tiles (3.6x fewer FLOPs).
        Every output element sees exactly the arithmetic of the per-tile pass (the reduction order of an output element does not
        depend on the tile it lies in), so the tiles are bit-identical; they are assembled in the reference's tile order and
        averaged by the same overlap kernel. Phase classes are dealt round-robin to the ranks.
        The tiles are those of hostio.tile_origins per axis (the x and y lists differ for H != W): a clamped last tile joins the class
        of its phase behind that class's regular tiles, or is a class of its own. A tile's sub-window sits at its origin minus the first
        origin of its run. `pps` (the tiles per side of a square image covered exactly) is implied by the image and accepted for callers
        that pass it.
        Returns float32 [n, nx, ny, P, P] indexed [image][x index][y index] (this rank's classes; zeros elsewhere)."""
        opts, net = self._options, self.net
        dev = net.device
        n, H, W = imgs_t.shape[0], imgs_t.shape[1], imgs_t.shape[2]
        P, S, L, stride = opts.patch_size, self.input_size, opts.num_layers, opts.stride
        off = (S - P) // 2
        period = 2 ** (L - 1)
        origins_x, origins_y = hostio.tile_origins(W, P, stride), hostio.tile_origins(H, P, stride)
        assert pps is None or (H == W and pps == len(origins_x) == len(origins_y))

        def mirror(length):
            # symmetric ("mirror_border", images.py:269-281) padding of any width by index arithmetic: period 2 * length
            m = torch.remainder(torch.arange(-off, length + off, device=dev), 2 * length)
            return torch.where(m < length, m, 2 * length - 1 - m)
        padded = imgs_t[:, mirror(H)][:, :, mirror(W)].contiguous()           # [n, Hp, Wp, 3]; windows reaching past it are zero-filled
        Hp, Wp = padded.shape[1], padded.shape[2]
        smax = int(os.environ.get("RSU_PREDICT_MAX_WINDOW", "1100"))   # largest input window (memory: ~1.7 GB per image at L = 6)

        def runs_of(origins):
            # per axis: the tile indices of each phase class in the order the classes first appear, cut into runs whose input window
            # S + (last origin - first origin) stays within smax (a run of one tile always fits)
            classes = {}
            for i, o in enumerate(origins):
                classes.setdefault(o % period, []).append(i)
            runs = []
            for cls in classes.values():
                run = [cls[0]]
                for i in cls[1:]:
                    if S + origins[i] - origins[run[0]] <= smax:
                        run.append(i)
                    else:
                        runs.append(run)
                        run = [i]
                runs.append(run)
            return runs
        tiles = torch.zeros((n, len(origins_x), len(origins_y), P, P), dtype=torch.float32, device=dev)   # [img][xi][yi] = the reference's tile order
        jobs = [(rx, ry) for rx in runs_of(origins_x) for ry in runs_of(origins_y)]
        bmax = max(1, int(os.environ.get("RSU_PREDICT_WINDOW_BATCH", "6")))   # ~2 GB of activations per window image at L = 6
        Bw = max(d for d in range(1, min(n, bmax) + 1) if n % d == 0)
        for ji, (rx, ry) in enumerate(jobs):
            if ji % self.world != self.rank:
                continue
            ox0, oy0 = origins_x[rx[0]], origins_y[ry[0]]
            Pk = P + max(origins_x[rx[-1]] - ox0, origins_y[ry[-1]] - oy0)
            wn = self._window_net(Pk, Bw)
            wn.ensure_tuned(training=False)   # the window nets have geometries of their own: one untimed tuning pass each
            Sk = wn.S
            h, w = min(Sk, Hp - oy0), min(Sk, Wp - ox0)
            for b0 in range(0, n, Bw):
                if h < Sk or w < Sk:
                    wn.x.zero_()
                wn.x[:, :h, :w] = padded[b0:b0 + Bw, oy0:oy0 + h, ox0:ox0 + w]
                wn.forward_device()
                for xi in rx:
                    for yi in ry:
                        dy, dx = origins_y[yi] - oy0, origins_x[xi] - ox0
                        tiles[b0:b0 + Bw, xi, yi] = wn.prob[:, dy:dy + P, dx:dx + P]
        return tiles

    def _window_net(self, Pk, Bw):
        """a forward-only network for a larger output window, sharing this model's current weights: flat_w, which inside
        net.averaged_weights() holds the averages -- the version key tells the two apart"""
        nets = self.__dict__.setdefault("_win_nets", {})
        opts = self._options
        wn = nets.get((Pk, Bw))
        if wn is None:
            wn = nets[Pk, Bw] = UNet(opts.num_layers, opts.root_size, opts.dilated_layers, Bw, Pk, device=self.net.device,
                                     params=None, seed=opts.seed, training=False)
            wn._weights_version = None
        ver = (self.net.global_step, getattr(self.net, "_load_count", 0), self.net._averaged)
        if wn._weights_version != ver:
            wn.flat_w.copy_(self.net.flat_w)
            wn.repack()
            wn._weights_version = ver
        return wn

    def predict_batchwise(self, imgs, pred_batch_size):
        """tf_aerial_images.py:330-341"""
        masks = []
        for i in range(int(np.ceil(imgs.shape[0] / pred_batch_size))):
            start = i * pred_batch_size
            masks.append(self.predict(imgs[start:start + pred_batch_size]))
        return np.concatenate(masks, axis=0) if len(masks) > 1 else masks[0]

    def quantize_mask(self, masks, threshold, patch_size):
        """images.quantize_mask (images.py:256-266) on the device: masks [n, H, W, 1] float -> same shape, every patch_size block
        overwritten with its label mean(mask >= 0.5) > threshold (a block cut by the image's edge: over the pixels it holds)"""
        a = np.asarray(masks)
        t = torch.as_tensor(np.ascontiguousarray(a[..., 0], dtype=np.float32)).to(self.net.device)
        p, st = mask_metrics.ptr(t), mask_metrics.stream(self.net.device)
        if t.shape[1] == t.shape[2]:
            call("rsu_quantize_mask", p, p, t.shape[0], t.shape[1], int(patch_size), float(threshold), st)
        else:
            call("rsu_quantize_mask_rect", p, p, t.shape[0], t.shape[1], t.shape[2], int(patch_size), float(threshold), st)
        return t.cpu().numpy()[..., None].astype(a.dtype)

    def postprocess_masks(self, masks, threshold=0.5):
        """The clean-up of predicted masks on the device (rsu_components_filter): masks [n, H, W, 1] probabilities -> the same shape and
        dtype, road components (p >= threshold at --component_connectivity) of fewer than --min_road_area pixels set to 0, then holes of
        at most --max_hole_area pixels set to 1, every other pixel unchanged. The identity -- `masks` itself, no launch -- when both flags
        are 0. Integer decisions on the same input: every rank computes the same bits. last_postprocess_stats holds the call's summed
        {components, components removed, pixels removed, holes, holes filled, pixels filled} (int64 [6]; None for the identity)."""
        opts = self._options
        min_area, max_hole = int(getattr(opts, "min_road_area", 0)), int(getattr(opts, "max_hole_area", 0))
        if min_area == 0 and max_hole == 0:
            self.last_postprocess_stats = None
            return masks
        a = np.asarray(masks)
        if a.ndim != 4 or a.shape[3] != 1:
            raise ValueError("postprocess_masks: masks must be [n, H, W, 1], not %s" % (a.shape,))
        n, H, W = (int(v) for v in a.shape[:3])
        dev = self.net.device
        ws = mask_metrics.workspace("components", (n, H, W), (), dev, "postprocess_masks: %d masks of %d x %d pixels are outside "
                                    "rsu_components.h's limits (H * W <= 2^24, n * H * W < 2^31): clean them in smaller stacks" % (n, H, W))
        t = torch.as_tensor(np.ascontiguousarray(a[..., 0], dtype=np.float32)).to(dev)
        stats = torch.empty((n, 6), dtype=torch.int64, device=dev)
        mask_metrics.components_filter(t, threshold, getattr(opts, "component_connectivity", 8), min_area, max_hole, t, stats, ws,
                                       mask_metrics.stream(dev))
        self.last_postprocess_stats = stats.sum(dim=0).cpu().numpy()
        return t.cpu().numpy()[..., None].astype(a.dtype)

    def centerlines(self, masks, threshold=0.5):
        """The centre-lines of predicted masks on the device (rsu_mask_thin with labels64 = NULL: every pixel counted): masks [n, H, W] or
        [n, H, W, 1] probabilities (what postprocess_masks returns) -> float32 [n, H, W], 1.0 on the one-pixel-wide, topology-preserving
        skeleton of {p >= threshold} and 0.0 elsewhere, after at most --centerline_max_iters iterations of Guo & Hall's thinning, and with
        --centerline_min_branch = L > 0 pruned of its branches of at most L pixels (rsu_skeleton_graph, in place on the skeletons).
        Integer decisions on the same input: every rank computes the same bits."""
        return self._centerlines_device(masks, threshold).cpu().numpy()

    def _centerlines_device(self, masks, threshold):
        """centerlines(), its result still on the device (mask_metrics.thin_stack)"""
        a = np.asarray(masks)
        if a.ndim == 4 and a.shape[3] == 1:
            a = a[..., 0]
        if a.ndim != 3:
            raise ValueError("centerlines: masks must be [n, H, W] or [n, H, W, 1], not %s" % (a.shape,))
        return mask_metrics.thin_stack(
            torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)), self.net.device, threshold, int(getattr(self._options, "centerline_max_iters", 64)), int(getattr(self._options, "centerline_min_branch", 0)),
            "centerlines (--save_centerlines): %d masks of %d x %d pixels are outside rsu_thin.h's limits (sides up to %d, n * H * W * 4 below "
            "2 GiB): thin them in smaller stacks" % (tuple(a.shape) + (THIN_MAX_SIDE,)))

    def road_graph(self, masks, threshold=0.5, distances=None):
        """The road network of predicted masks, one plain dict per image (hostio.road_graph: nodes and edges with their lengths): masks
        [n, H, W] or [n, H, W, 1] probabilities -> the centre-lines of {p >= threshold} (rsu_mask_thin, pruned by --centerline_min_branch:
        centerlines()), cut at their junctions into segments and measured on the device (rsu_line_segments, --max_segments rows per
        image; a dict carries "segments" = the true segment count, which may exceed its edges). Integer decisions on the same input:
        every rank computes the same network. With --road_graph_paths the segment labels are asked for too, rsu_segment_paths orders the
        pixels of every stored segment of at most --max_path_length pixels along it, every edge gains "kind" and "path" (hostio.road_graph,
        simplified at --road_graph_simplify) and every dict "unordered" = its branched and too long segments. With distances=True
        (None: --road_graph_distances) rsu_graph_routes runs on the same tables and every dict gains "node_index", the node ids in the
        order of the device's node table (--max_graph_nodes rows; "nodes_dropped" = those past it), and "distances", the length in
        pixels (w / 70) of the shortest path between every two of them, row-major over node_index, None where there is no path."""
        lines = self._centerlines_device(masks, threshold)   # (exactly 0.0 / 1.0, and they stay on the device)
        n, H, W = (int(v) for v in lines.shape)
        opts = self._options
        cap, dev, st = int(getattr(opts, "max_segments", 4096)), lines.device, mask_metrics.stream(lines.device)
        ws = mask_metrics.workspace("segments", (n, H, W), (cap,), dev, "road_graph (--save_road_graph): %d masks of %d x %d pixels are outside "
                                    "rsu_segments.h's limits (sides up to %d, n * H * W * 16 below 2 GiB): use smaller stacks"
                                    % (n, H, W, SEGMENTS_MAX_SIDE))

        def zeros(*shape):
            return torch.zeros(shape, dtype=torch.int32, device=dev)

        edges, counts, node = zeros(n, cap, 8), zeros(n, 4), zeros(n, H, W)
        ordered = bool(getattr(opts, "road_graph_paths", False))
        seg = zeros(n, H, W) if ordered else None
        mask_metrics.line_segments(lines, 0.5, None, cap, edges, None, counts, seg, None, node, None, None, ws, st)
        if ordered:
            max_len, eps = int(getattr(opts, "max_path_length", 4096)), float(getattr(opts, "road_graph_simplify", 0.0))
            pws = mask_metrics.workspace("paths", (n, H, W), (cap, max_len), dev, "road_graph (--road_graph_paths): %d masks of %d x %d pixels "
                                         "are outside rsu_paths.h's limits (sides up to %d, n * H * W * 16 below 2 GiB): use smaller stacks"
                                         % (n, H, W, PATHS_MAX_SIDE))
            paths, offsets, kind, info = zeros(n, H * W), zeros(n, cap + 1), zeros(n, cap), zeros(n, 4)
            mask_metrics.segment_paths(seg, edges, counts, 0, max_len, H * W, paths, offsets, kind, None, info, pws, st)
            paths, offsets, kind, info = (t.cpu().numpy() for t in (paths, offsets, kind, info))
        routed = bool(getattr(opts, "road_graph_distances", False)) if distances is None else bool(distances)
        if routed:
            cap_nodes = int(getattr(opts, "max_graph_nodes", 256))
            rws = mask_metrics.workspace("routes", (n, H, W), (cap_nodes,), dev, "road_graph (--road_graph_distances): %d masks of %d x %d "
                                         "pixels with %d nodes each are outside rsu_routes.h's limits (sides up to %d, n * max_graph_nodes^2 * 4 "
                                         "below 2 GiB): use smaller stacks" % (n, H, W, cap_nodes, ROUTES_MAX_SIDE))
            rt_nodes, rt_dist, rt_info = zeros(n, cap_nodes, 4), zeros(n, cap_nodes, cap_nodes), zeros(n, 4)
            mask_metrics.graph_routes(node, edges, counts, 0, rt_nodes, rt_dist, rt_info, rws, st)
            rt_nodes, rt_dist, rt_info = (t.cpu().numpy() for t in (rt_nodes, rt_dist, rt_info))
        edges, counts, node = edges.cpu().numpy(), counts.cpu().numpy(), node.cpu().numpy()
        out = []
        for i in range(n):
            g = hostio_road_graph(edges[i], int(counts[i, 0]), node[i], H, W, paths=(paths[i], offsets[i], kind[i]) if ordered else None)
            g["segments"] = int(counts[i, 0])
            if ordered:
                g["unordered"] = int(info[i, 3])
                for e in g["edges"] if eps > 0.0 else ():
                    if len(e["path"]) > 2:
                        e["path"] = simplify_path(np.asarray(e["path"], np.int64), eps).tolist()
            if routed:
                k = int(rt_info[i, 1])
                g["node_index"] = [int(v) for v in rt_nodes[i, :k, 0]]
                g["nodes_dropped"] = int(rt_info[i, 0]) - k
                g["distances"] = [[None if int(v) >= ROUTES_INF else int(v) / 70.0 for v in row] for row in rt_dist[i, :k, :k]]
            out.append(g)
        return out

    # ------------------------------------------------------------------ checkpoints
    def save_as(self, path):
        """tf_aerial_images.py:458: the saver writing to an explicit path (`path`.npz: every variable under its TF name and layout,
        its optimizer slots (UNet.state_dict) and global_step; '/' in a name is stored as '|' -- np.savez keys become file names)"""
        if self.rank == 0:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.savez(path + ".npz", **{k.replace("/", "|"): v for k, v in self.net.state_dict().items()})
        return path

    def save(self, epoch=0):
        """tf_aerial_images.py:343-349: {save_path}/{experiment_name}/model-epoch-{epoch:03d}.chkpt(.npz)"""
        opts = self._options
        path = self.save_as(os.path.abspath(os.path.join(opts.save_path, self.experiment_name, 'model-epoch-{:03d}.chkpt'.format(epoch))))
        if self.rank == 0:
            print("Model saved in file: {}".format(path))
        return path

    def restore_from_tf_arrays(self, arrays):
        """Load a checkpoint of the REFERENCE: `arrays` maps TensorFlow variable names to numpy arrays, as written by
        tools/export_tf_checkpoint.py on a machine that has TensorFlow (tf.train.load_checkpoint(...).get_tensor(name) for every
        name; tf_aerial_images.py:171 saves all global variables). Names and layouts are the reference's own, so this is a pure
        rename: `<var>` -> weights, `<var>/Momentum` -> optimizer slots, `global_step` (tf_aerial_images.py:113) -> step counter; a run
        with tf.train.AdamOptimizer: `<var>/Adam`, `<var>/Adam_1`, `beta1_power`, `beta2_power` (read by an Adam model; UNet.load_state_dict);
        a run with tf.train.ExponentialMovingAverage: `<var>/ExponentialMovingAverage` (read by a model with --ema_decay).
        A ':0' suffix and a leading scope are tolerated; missing variables raise KeyError."""
        clean = {}
        for k, v in arrays.items():
            k = k[:-2] if k.endswith(":0") else k
            clean[k] = np.asarray(v)
        d = {}
        for n in self.net.names:
            hit = [k for k in clean if k == n or k.endswith("/" + n)]
            if not hit:
                raise KeyError("variable %r not found in the exported checkpoint" % n)
            d[n] = clean[hit[0]]
            if d[n].shape != tuple(self.net.w[n].shape):
                raise ValueError("variable %r: checkpoint shape %s, network %s" % (n, d[n].shape, tuple(self.net.w[n].shape)))
            for slot in ("/Momentum", "/Adam", "/Adam_1", EMA_SUFFIX):
                hit = [k for k in clean if k == n + slot or k.endswith("/" + n + slot)]
                if hit:
                    d[n + slot] = clean[hit[0]]
        for scalar in ("beta1_power", "beta2_power"):
            hit = [k for k in clean if k == scalar or k.endswith("/" + scalar)]
            if hit:
                d[scalar] = np.float32(clean[hit[0]])
        gs = [k for k in clean if k == "global_step" or k.endswith("/global_step")]
        d["global_step"] = int(clean[gs[0]]) if gs else 0
        self.net.load_state_dict(d)

    def restore(self, date=None, epoch=None, file=None):
        """Restores model from saved checkpoint (tf_aerial_images.py:351-379): explicit file, else newest experiment
        directory under save_path (or `date`), newest epoch (or `epoch`). As in the reference (tf_aerial_images.py:360), with
        date=None EVERY directory under save_path takes part in the "newest by name" choice, experiment directory or not."""
        opts = self._options
        if file is not None:
            model_data_dir = file
        else:
            if date is None:
                dates = [d for d in glob.glob(os.path.join(opts.save_path, "*")) if os.path.isdir(d)]
                model_data_dir = sorted(dates)[-1]
            else:
                model_data_dir = os.path.abspath(os.path.join(opts.save_path, date))
            if epoch is None:
                model_data_dir = sorted(glob.glob(os.path.abspath(os.path.join(model_data_dir, 'model-epoch-*.chkpt.npz'))))[-1][:-4]
            else:
                model_data_dir = os.path.abspath(os.path.join(model_data_dir, 'model-epoch-{:03d}.chkpt'.format(epoch)))
        path = model_data_dir if model_data_dir.endswith(".npz") else model_data_dir + ".npz"
        with np.load(path) as z:
            self.net.load_state_dict({k.replace("|", "/"): z[k] for k in z.files})
        print("Model restored from from file: {}".format(model_data_dir))
