"""Drop-in for DenseFusion/replace_ycb_toolbox: the two scripts of the YCB-Video toolbox that turn the `poses` files of
tools/eval_ycb.py into the benchmark's figures (ADD-S / ADD AUC and the share below 2 cm), without MATLAB.  `main` runs the three steps."""


def main(dataset_root, model, refine_model, ycb_toolbox_dir="YCB_Video_toolbox", dataset_config_dir="datasets/ycb/dataset_config",
         result_wo_refine_dir="experiments/eval_result/ycb/Densefusion_wo_refine_result",
         result_refine_dir="experiments/eval_result/ycb/Densefusion_iterative_result", out="results_keyframe.mat", frames=None,
         device="cuda:0", verbose=True, **eval_kwargs):
    """tools/eval_ycb.main over `frames` of the test list (None: all), evaluate_poses_keyframe over the files it wrote, plot_accuracy_keyframe
    over the result; prints the legends' table -> (results, figures)"""
    from autoposeestimation_amd.DenseFusion.tools import eval_ycb
    from .evaluate_poses_keyframe import evaluate_poses_keyframe, read_lines
    from .plot_accuracy_keyframe import legend_table, plot_accuracy_keyframe
    import os
    eval_ycb.main(dataset_root, model, refine_model, ycb_toolbox_dir=ycb_toolbox_dir, dataset_config_dir=dataset_config_dir,
                  result_wo_refine_dir=result_wo_refine_dir, result_refine_dir=result_refine_dir, frames=frames, device=device, **eval_kwargs)
    results = evaluate_poses_keyframe(dataset_root, ycb_toolbox_dir, result_refine_dir, result_wo_refine_dir, dataset_config_dir=dataset_config_dir,
                                      keyframes=frames, out=out, device=device)
    figures = plot_accuracy_keyframe(results, read_lines(os.path.join(dataset_config_dir, "classes.txt")))
    if verbose:
        for line in legend_table(figures):
            print(line)
    return results, figures
