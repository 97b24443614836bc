"""Command-line surface of the reference's src/tf_aerial_images.py (flags :15-46, main :382-466) over the HIP path.

    python -m road_segmentation_unet_amd.cli --num_layers=5 --root_size=64 --patch_size=388 --dilated_layers ...
    torchrun --nproc-per-node 8 -m road_segmentation_unet_amd.cli ...     (data-parallel: --batch_size is the global batch)

Boolean flags follow tf.app.flags: `--flag`, `--flag=true|false`, `--noflag`."""
import argparse
import os
import sys
import time

import numpy as np


def build_parser():
    from .model import EXTRA_FLAG_DEFS, FLAG_DEFS
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, typ, default, helptext in FLAG_DEFS + EXTRA_FLAG_DEFS:
        if typ is bool:
            ap.add_argument("--" + name, nargs="?", const=True, default=default,
                            type=lambda s: s.lower() in ("1", "true", "t", "yes", "y"), help=helptext)
            ap.add_argument("--no" + name, dest=name, action="store_false", help=argparse.SUPPRESS)
        else:
            ap.add_argument("--" + name, type=typ, default=default, help=helptext)
    return ap


def parse_options(argv=None):
    from .model import Options
    ns = build_parser().parse_args(argv)
    return Options(**vars(ns))


def _clean_up(model, masks, threshold, rank):
    """--min_road_area / --max_hole_area between prediction and quantisation: postprocess_masks and one line with the summed stats"""
    masks = model.postprocess_masks(masks, threshold=threshold)
    stats = model.last_postprocess_stats
    if stats is not None and rank == 0:
        print("Mask clean-up: {} components, {} removed ({} pixels); {} holes, {} filled ({} pixels)".format(*[int(v) for v in stats]))
    return masks


def main(argv=None):
    import torch
    import torch.distributed as dist
    from . import hostio
    from .model import ConvolutionalModel, balanced_class_weights
    from .pool import DevicePatchPool
    from .unet import input_size_needed
    opts = parse_options(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not dist.is_initialized():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
    rank = dist.get_rank() if dist.is_initialized() else 0
    train_data = None
    if opts.validation_images > 0 and opts.num_epoch > 0:
        # whole images leave the training set before anything is derived from it (the balanced class weights, rotation, patches)
        train_data, held_out = hostio.split_validation(*hostio.load_train_data(opts.train_data_dir), opts.validation_images)
    else:
        held_out = None
    if opts.class_weights == "balanced":
        # the model takes its class weights at construction: this case alone loads the training set in front of it. Without a
        # training epoch the loss is never evaluated and the flag has no effect
        if opts.num_epoch > 0:
            train_data = train_data if train_data is not None else hostio.load_train_data(opts.train_data_dir)
            opts.class_weights = balanced_class_weights(train_data[1])
            print("Balanced class weights: background {:.4f}, road {:.4f}".format(*opts.class_weights))
        else:
            opts.class_weights = None
    model = ConvolutionalModel(opts)
    print("Running on device {}".format(model.net.device))
    if opts.weight_decay > 0.0:
        decays, live = model.net.decaying_parameters()
        print("Weight decay: {} lambda {:g}, {} of {} live parameters decay (conv kernels; biases, colour adjust and the head do not); "
              "the reported loss excludes the penalty".format(opts.weight_decay_mode, opts.weight_decay, decays, live))
    if opts.focal_gamma > 0.0:
        print("Focal loss: gamma {:g}; the logged loss and the validation loss / objective are the focal objective, and the gradient is "
              "smaller than the cross-entropy's (--lr is not rescaled)".format(opts.focal_gamma))

    if opts.cldice_weight > 0.0:
        print("clDice term: lambda {:g}, {} erosions, smooth {:g}; the logged loss and the validation objective include lambda * (1 - clD)"
              .format(opts.cldice_weight, opts.cldice_iters, opts.cldice_smooth))

    if opts.lovasz_weight > 0.0:
        print("Lovasz term: lambda {:g}; the logged loss and the validation objective include lambda * the mean per-image Lovasz "
              "(Jaccard surrogate) loss".format(opts.lovasz_weight))

    if opts.min_road_area > 0 or opts.max_hole_area > 0:
        print("Mask clean-up: road components below {} pixels removed ({}-connected), holes of at most {} pixels filled, before the masks "
              "are quantised".format(opts.min_road_area, opts.component_connectivity, opts.max_hole_area))

    if opts.restore_model:
        if opts.model_path is not None:
            model.restore(file=opts.model_path)
            print("Restore model: {}".format(opts.model_path))
        else:
            print("Restore date: {}".format(opts.restore_date))
            model.restore(date=opts.restore_date, epoch=opts.restore_epoch)

    if opts.num_epoch > 0:
        train_images, train_groundtruth = train_data if train_data is not None else hostio.load_train_data(opts.train_data_dir)
        input_size = input_size_needed(opts.patch_size, opts.num_layers)
        offset = int((input_size - opts.patch_size) / 2)
        extended = hostio.expand_and_rotate(train_images, opts.rotation_angles, offset)
        gt_exp = hostio.expand_and_rotate(train_groundtruth, opts.rotation_angles, 0)
        if opts.device_patch_pool:
            # the reference's extract_patches arrays as an index over the rotated images, resident in HBM (pool.DevicePatchPool):
            # same patches, same order, no 30-GB float64 pool on the host and no upload per step
            patches = DevicePatchPool(extended, gt_exp, input_size, opts.patch_size, opts.stride, device=model.net.device,
                                      augment=opts.d4_augmentation, seed=opts.seed, rotation=opts.random_rotation,
                                      scale=opts.random_scale, one_launch=opts.one_launch_loader, jitter=opts.color_jitter,
                                      noise=opts.random_noise, elastic=opts.elastic_deformation)
            labels_patches = None
            print("Train on {} patches of size {}x{}".format(patches.shape[0], patches.shape[1], patches.shape[2]))
            print("Train on {} groundtruth patches of size {}x{}".format(patches.shape[0], opts.patch_size, opts.patch_size))
        else:
            patches = hostio.extract_patches(extended, patch_size=input_size, predict_patch_size=opts.patch_size, stride=opts.stride)
            print("Train on {} patches of size {}x{}".format(patches.shape[0], patches.shape[1], patches.shape[2]))
            labels_patches = hostio.extract_patches(gt_exp, patch_size=opts.patch_size, stride=opts.stride)
            print("Train on {} groundtruth patches of size {}x{}".format(*labels_patches.shape[:3]))
        if opts.lr_schedule in ("cosine", "linear"):
            given = opts.lr_total_steps
            total = model.resolve_lr_total_steps(patches.shape[0])
            print("Learning-rate schedule: {} over {} optimizer steps{}, warm-up {} steps, final {:g} x lr".format(
                opts.lr_schedule, total, "" if given else " ({} epoch(s) x {} steps)".format(opts.num_epoch, total // opts.num_epoch),
                opts.lr_warmup_steps, opts.lr_final))
        validation = None
        if held_out is not None:
            validation = hostio.validation_patches(held_out[0], held_out[1], input_size, opts.patch_size)
            print("Validate on {} patches of {} held-out images".format(validation[0].shape[0], len(held_out[0])))
        summary = model._ensure_summary()
        if summary is not None:
            summary.add_to_eval_patch_summary(train_groundtruth)
        for i in range(opts.num_epoch):
            print("==== Train epoch: {} ====".format(i))
            if summary is not None:
                summary.reset()  # tf.local_variables_initializer().run(): reset scores
            stats = model.train(patches, labels_patches, train_images, train_groundtruth, validation=validation)
            if rank == 0:
                print("\nepoch {} : {}".format(i, stats))
            model.save(i)

    if opts.eval_train:
        # tf_aerial_images.py:432-445: predict the training images and dump five picture sets next to each other (file names as the
        # reference writes them, its "eval_orror" included, so that its downstream scripts keep finding them)
        print("Evaluate Test")
        eval_images, eval_groundtruth = hostio.load_train_data(opts.train_data_dir)
        probabilities = _clean_up(model, model.predict_batchwise(eval_images, opts.pred_batch_size), 0.5, rank)
        if rank == 0:
            binary = ((probabilities > 0.5) * 1).squeeze(-1)
            dumps = (
                ("eval_binary_pred_{:03d}.png", binary, True),
                ("eval_probability_pred_{:03d}.png", probabilities, True),
                ("eval_overlays_pred_{:03d}.png", hostio.overlays(eval_images, probabilities, fade=0.5), False),
                ("eval_confusion_{:03d}.png", hostio.overlap_pred_true(binary, eval_groundtruth), False),
                ("eval_orror_{:03d}.png", hostio.overlapp_error(binary, eval_groundtruth), True),
            )
            for pattern, pictures, grey in dumps:
                hostio.save_all(pictures, opts.eval_data_dir, pattern, greyscale=grey)

    if opts.eval_data_dir and not opts.eval_train:
        print("Running inference on eval data {}".format(opts.eval_data_dir))
        eval_images = hostio.load(opts.eval_data_dir)   # one common shape, any H x W (ValueError for a directory of mixed shapes)
        start = time.time()
        masks = model.predict_batchwise(eval_images, opts.pred_batch_size)
        print("Prediction time:{} mins".format((time.time() - start) / 60))
        masks = _clean_up(model, masks, 0.5, rank)   # (quantize_mask binarises at 0.5 before it averages a block)
        lines = model.centerlines(masks, threshold=0.5) if opts.save_centerlines else None   # (of the cleaned masks, before they are quantised)
        graphs = model.road_graph(masks, threshold=0.5) if opts.save_road_graph else None   # (of the cleaned masks too)
        masks = model.quantize_mask(masks, patch_size=hostio.IMG_PATCH_SIZE, threshold=hostio.FOREGROUND_THRESHOLD)
        if rank == 0:
            save_dir = os.path.abspath(os.path.join(opts.save_path, model.experiment_name))
            overlays = hostio.overlays(eval_images, masks, fade=0.4)
            hostio.save_all(overlays, save_dir)
            if lines is not None:
                hostio.save_all(lines, save_dir, "centerlines_{:03d}.png", greyscale=True)
                print("Centre-lines: {} skeleton pixels in {} images".format(int(lines.sum()), len(lines)))
            if graphs is not None:
                import json
                for i, g in enumerate(graphs):   # (numbered as save_all numbers the overlays)
                    with open(os.path.join(save_dir, "graph_{:03d}.json".format(i + 1)), "w") as f:
                        json.dump(g, f)
                print("Road graphs: {} nodes and {} edges in {} images".format(sum(len(g["nodes"]) for g in graphs),
                                                                               sum(len(g["edges"]) for g in graphs), len(graphs)))
                if opts.road_graph_paths:
                    print("Road paths: {} points, {} segments not ordered (branched or longer than {} pixels)".format(
                        sum(len(e["path"]) for g in graphs for e in g["edges"]), sum(g["unordered"] for g in graphs), opts.max_path_length))
                if opts.road_graph_distances:
                    print("Road distances: {} nodes in the tables, {} past --max_graph_nodes={}".format(
                        sum(len(g["node_index"]) for g in graphs), sum(g["nodes_dropped"] for g in graphs), opts.max_graph_nodes))
            if masks.shape[1] % hostio.IMG_PATCH_SIZE or masks.shape[2] % hostio.IMG_PATCH_SIZE:
                print("No submission.csv: {} x {} images are not made of whole {}-pixel patches".format(
                    masks.shape[1], masks.shape[2], hostio.IMG_PATCH_SIZE))
            else:
                hostio.save_submission_csv(masks, save_dir, hostio.IMG_PATCH_SIZE)
            model.save_as(save_dir + "-model.chkpt")  # the model used for the submission
    if dist.is_initialized():
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
