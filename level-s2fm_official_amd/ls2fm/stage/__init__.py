"""The stage drivers of the reference as loops over one optimisation step:

    step.py     the step itself: `render_losses`, `surface_losses`, `RenderStage` (eager, or captured into one hipGraph)
    terms.py    the loss terms formed outside the render as fused autograd nodes: `reprojection_term`, `host_intrinsic`
    loops.py    the scene container `TrackedViews`, `keypoint_rays`, `TracingConsistency` and the loops: five over the step, `TradBALoop` (Adam) and
                `LMBALoop` (Levenberg-Marquardt with a Schur complement) over explicit points and poses
"""
from .loops import BALoop, GeoInitLoop, InitLoop, LMBALoop, RefineLoop, TracingConsistency, TrackedViews, TradBALoop, keypoint_rays  # noqa: F401
from .step import RenderStage, render_losses, surface_losses  # noqa: F401
from .terms import host_intrinsic, reprojection_term  # noqa: F401
