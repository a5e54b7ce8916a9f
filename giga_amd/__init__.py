"""giga_amd: MI355X-native (gfx950) implementation of GIGA's dense inference path.

    from giga_amd.networks import get_network, load_network     # vgn.networks drop-in (GIGA entries)
    from giga_amd.detection import query_lattice, predict       # vgn.detection_implicit counterpart
    from giga_amd import render_depth, acquire_tsdf, save_occ   # depth images and occupancy labels from meshes (giga_amd.render)
    from giga_amd import ResidentTrainingSet, ResidentBatches   # training batches from a set in device memory (giga_amd.resident)
    from giga_amd import Trainer, train_val_split               # the training loop of scripts/train_giga.py (giga_amd.trainer)
    from giga_amd import GeoTrainer, geo_loss                   # ... and of scripts/train_giga_geo.py: the occupancy-only giga_geo
    from giga_amd import affordance_visual, grasp2mesh          # the scene mesh coloured by grasp quality (giga_amd.visual)
    from giga_amd import render_color, render_mesh, write_png   # shaded images of coloured meshes (giga_amd.render, giga_amd.visual)
    from giga_amd import GeometryEvaluator, VoxelOccGeoROIDataset   # scene IoU, chamfer, grasp-ROI occupancy (giga_amd.geometry)
    from giga_amd import mesh_collide, generate_packed_scenes, write_geo_dataset   # packed scenes from object meshes (giga_amd.scenes)
    from giga_amd import grasp_candidates, reduce_outcomes      # grasp candidates from the oriented TSDF cloud (giga_amd.candidates)

All arithmetic runs in hand-written HIP kernels behind the C ABI of include/giga_hip.h."""
__version__ = "0.1.0"

# names of giga_amd.render, resolved on first use (importing the package stays free of torch)
_RENDER_EXPORTS = ("scene_mesh", "Camera", "render_depth", "render_depth_batch", "acquire_tsdf", "acquire_tsdfs", "write_raw_scenes",
                   "sample_iou_points", "save_occ", "render_color", "render_color_batch")
# ... and of giga_amd.resident: the training set in device memory and its batch iterator
_RESIDENT_EXPORTS = ("ResidentTrainingSet", "ResidentBatches")
# ... and of giga_amd.trainer: the training loop, its device-side epoch metrics and the train / validation split
_TRAINER_EXPORTS = ("Trainer", "TrainMetrics", "train_val_split", "GeoTrainer", "geo_loss")
# ... and of giga_amd.visual: the affordance colours of a scene mesh, the gripper glyph, the composed scene
_VISUAL_EXPORTS = ("affordance_faces", "affordance_points", "affordance_visual", "grasp2mesh", "ColoredMesh", "Scene", "render_mesh",
                   "get_camera_pose", "look_at", "extrinsic_from_camera_pose", "write_png")
# ... and of giga_amd.geometry: the scoring of predicted geometry (scene IoU, chamfer, grasp-ROI occupancy) and its data sets
_GEOMETRY_EXPORTS = ("GeometryEvaluator", "VoxelOccGeoDataset", "VoxelOccGeoROIDataset", "occ_confusion", "occ_scores",
                     "roi_point_counts", "load_obj", "default_mesh_loader", "read_mesh_pose_list")
# ... of giga_amd.collision (do two meshes intersect?) and of giga_amd.scenes (packed scenes and the geometry data set they make)
_COLLISION_EXPORTS = ("mesh_collide", "mesh_bounds_batch")
_SCENES_EXPORTS = ("ObjectSet", "packed_candidates", "resolve_packed", "generate_packed_scenes", "table_mesh", "write_geo_dataset")
# ... and of giga_amd.candidates: grasp candidates from the oriented TSDF cloud and the reduction of an executor's outcomes
_CANDIDATES_EXPORTS = ("workspace_bounds", "grasp_candidates", "reduce_outcomes", "label_scenes", "scene_views")


def __getattr__(name):
    if name in _RENDER_EXPORTS:
        from . import render
        return getattr(render, name)
    if name in _RESIDENT_EXPORTS:
        from . import resident
        return getattr(resident, name)
    if name in _TRAINER_EXPORTS:
        from . import trainer
        return getattr(trainer, name)
    if name in _VISUAL_EXPORTS:
        from . import visual
        return getattr(visual, name)
    if name in _GEOMETRY_EXPORTS:
        from . import geometry
        return getattr(geometry, name)
    if name in _COLLISION_EXPORTS:
        from . import collision
        return getattr(collision, name)
    if name in _SCENES_EXPORTS:
        from . import scenes
        return getattr(scenes, name)
    if name in _CANDIDATES_EXPORTS:
        from . import candidates
        return getattr(candidates, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
