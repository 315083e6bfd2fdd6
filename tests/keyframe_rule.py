"""The keyframe rule of ea_tracker_batch_set_keyframes restated from the comments of include/ea_hip.h, for the tests that
compare the library with it (test_keyframe_decide_host.py, test_gpu_tracker_keyframes.py).  Python floats are IEEE doubles:
each comparison below has the one multiplication the header writes."""

KEY_FIRST, KEY_SOLVE_FAILED, KEY_VISIBLE, KEY_INLIERS, KEY_FLOW, KEY_AGE = 1, 2, 4, 8, 16, 32


def keyframe_decide(stats, params, age, aligned, failed):
    """stats: dict n, n_visible, n_inlier, n_flow, sum_flow; params: dict of ea_keyframe_params' fields; age: frames solved
    against the keyframe, this one included.  Returns the reason mask, 0 = keep."""
    if not aligned:
        return KEY_FIRST
    if failed:
        return KEY_SOLVE_FAILED
    why = 0
    n = float(stats["n"])
    if params["min_visible_fraction"] > 0.0 and float(stats["n_visible"]) < params["min_visible_fraction"] * n:
        why |= KEY_VISIBLE
    if params["min_inlier_fraction"] > 0.0 and float(stats["n_inlier"]) < params["min_inlier_fraction"] * n:
        why |= KEY_INLIERS
    if params["max_mean_flow"] > 0.0 and stats["n_flow"] > 0 and stats["sum_flow"] > params["max_mean_flow"] * float(stats["n_flow"]):
        why |= KEY_FLOW
    if params["max_frames"] > 0 and age >= params["max_frames"]:
        why |= KEY_AGE
    return why
