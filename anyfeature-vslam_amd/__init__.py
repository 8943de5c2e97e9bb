"""anyfeature-vslam_amd — MI355X-native ORB32 extraction + descriptor matching behind AnyFeature-VSLAM's
FeatureExtractor / FeatureMatcher interface.  (The directory name carries a hyphen: import it with
importlib.import_module("anyfeature-vslam_amd").)

Layout:
  csrc/          hand-written HIP kernels for gfx950 + the C-ABI runtime (libafv_hip.so, include/afv_hip.h)
  adapter/       C++ host adapter mirroring the reference's classes on top of the C-ABI
  _lib.py        ctypes binding
  extractor.py   FeatureExtractorSettings / FeatureExtractor_orb32 mirror (reference: Feature_orb32.{h,cpp})
  matcher.py     FeatureMatcher mirror (reference: FeatureMatcher.{h,cc})
  frame.py       the device-resident Frame (reference: Frame.{h,cc} as far as the front end reads it)
  points.py      the device-resident map-point store (reference: MapPoint.{h,cc} as far as the projection searches read it)
  database.py    KeyFrameDatabase mirror over the keyframe table (reference: KeyFrameDatabase.{h,cc}, LoopClosing.cc:137-157)
  sim3.py        Sim3Solver mirror: all RANSAC hypotheses of a loop check in one device call (reference: Sim3Solver.{h,cc});
                 OptimizeSim3 / OptimizeSim3Batch: Optimizer::OptimizeSim3 for every candidate in one device call
  lba.py         LocalBundleAdjustment / BundleAdjustment over table slots and store ids (reference: Optimizer.cc:450-768, :61-243);
                 GlobalBundleAdjustment: the block-sparse route for the whole map (Optimizer.cc:53-58, LoopClosing.cc:664)
  refresh.py     RefreshMapPoints: ComputeDistinctiveDescriptors and UpdateNormalAndDepth of resident map points from the observation list
                 of the bundle adjustment (reference: MapPoint.cc:279-349, :372-418)
  covisibility.py the covisibility count and the local map from the table's map-point planes (include/afv_covis.h) and CovisibilityGraph, the
                 host mirror of UpdateConnections and Tracking::UpdateLocalMap (reference: KeyFrame.cc:131-219, :329-418, Tracking.cc:1040-1144)
  essgraph.py    OptimizeEssentialGraph over plain arrays and the store, the edge list of the essential graph, the Sim3 point correction
                 (reference: Optimizer.cc:771-1031, LoopClosing.cc:487-516)
  pnp.py         PnPsolver mirror: all EPnP RANSAC hypotheses of a relocalisation in one device call (reference: PnPsolver.{h,cc})
  initializer.py Initializer mirror: H and F RANSAC and the reconstruction in one device call (reference: Initializer.{h,cc})
  synth.py       bit-reproducible synthetic inputs
"""
from . import _lib, synth  # noqa: F401
from .extractor import (CovarianceMethod, FeatureExtractorSettings, FeatureExtractor_orb32, Context,  # noqa: F401
                        KP_DTYPE)
from .vocabulary import Vocabulary  # noqa: F401
from .frame import Frame  # noqa: F401
from .points import MapPoints  # noqa: F401
from . import akaze, table  # noqa: F401
from .database import KeyFrameDatabase  # noqa: F401
from . import covisibility  # noqa: F401
from .covisibility import CovisibilityGraph, covisibility_votes, local_points  # noqa: F401
from .sim3 import OptimizeSim3, OptimizeSim3Batch, Sim3Solver  # noqa: F401
from .lba import BundleAdjustment, GlobalBundleAdjustment, LocalBundleAdjustment  # noqa: F401
from .essgraph import OptimizeEssentialGraph, essential_graph_edges  # noqa: F401
from .initializer import Initializer  # noqa: F401
from .pnp import PnPsolver  # noqa: F401
from .akaze import AkazeContext  # noqa: F401
from .matcher import (FeatureMatcher, FeatureView, FrameGridView, ProjectionQueries,  # noqa: F401
                      DescriptorDistance_orb32, DescriptorDistance_sift128)
# ComputeDistinctiveDescriptors(ctx, descriptor_sets) stays the form over host rows (matcher.py); with a table in front it is the resident one
from .refresh import (ComputeDistinctiveDescriptors, RefreshAfterBundleAdjustment, RefreshMapPoints, UpdateNormalAndDepth)  # noqa: F401
