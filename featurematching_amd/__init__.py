"""featurematching_amd - MI355X-native coarse-to-fine feature matching hot path."""
__version__ = "0.1.0"

# the validation step's names (post.py), resolved on first use so that importing the package stays free of torch
_POST = ("estimate_poses", "estimate_pose", "relative_pose_error", "compute_pose_errors", "error_auc", "epidist_prec",
         "aggregate_metrics", "compute_symmetrical_epipolar_errors")


def __getattr__(name):
    if name in _POST:
        from . import post
        return getattr(post, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
