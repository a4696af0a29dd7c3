"""shapemol_amd -- MI355X-native (gfx950) implementation of ShapeMol's denoising hot path.

Public surface (mirrors the reference's models/molopt_score_model.py):
    ScorePosNet3D, log_sample_categorical, pointcloud_shape_guidance, mesh_shape_guidance
and, outside it, the frozen shape encoder that produces the conditioning (models/shape_pointcloud_modelAE.py):
    VN_DGCNN_Encoder
and the auto-encoder it is half of, with the decoder that evaluates the field a latent encodes:
    PointCloud_AE, DecoderInner      (training: DecoderInner.train_field, PointCloud_AE.get_generator_train_loss)
and the builder of its training batches and of the sampling script's shape conditions, from molecule meshes (datasets/shape_data.py,
utils/shape.py):
    ShapeData, collate_fn, get_pointAE_shape_emb
and the molecule meshes themselves, from atom coordinates and radii (utils/shape.py get_mesh; the surface rule is this package's):
    get_mesh, get_mesh_batch
and, after the chain, the scores of sampled molecules that need no chemistry toolkit (utils/evaluation analyze.check_stability,
eval_bond_length pair-distance profiles), for one frame or every recorded frame, with the rule given as data:
    StabilityRule, GeometryReport, check_stability, evaluate_geometry, evaluate_trajectory, evaluate_samples
and how well a sample matches the shape of its condition (utils/evaluation shaep_utils.get_ROCS / shape_tanimoto, espsim's Gaussian
integrals, calculate_shaep_shape_sim with this package's own overlay in place of the ShaEP executable):
    shape_tanimoto, get_rocs, esp_similarity, align_shapes, similarity_to_condition
and the molecular graph of a sample under the same distance rule -- bonds with orders, fragments, completeness, rings, bond-length
profiles (the rule is this package's, not OpenBabel's perception; agreement with the reference's reconstruction is not measured):
    GraphReport, bond_graph, bond_graph_trajectory, bond_graph_samples, atom_type_jsd, to_molblock
plus helpers: synthetic weights/inputs (synth), schedules (diffusion), the C-ABI binding (_lib).
"""
from .molopt_score_model import ScorePosNet3D, log_sample_categorical, pointcloud_shape_guidance, mesh_shape_guidance  # noqa: F401
from .packing import pack_state_dict  # noqa: F401
from .shape_encoder import VN_DGCNN_Encoder  # noqa: F401
from .shape_autoencoder import PointCloud_AE, DecoderInner  # noqa: F401
from .shape_data import ShapeData, collate_fn, get_pointAE_shape_emb  # noqa: F401
from .mol_surface import get_mesh, get_mesh_batch  # noqa: F401
from .evaluation import (StabilityRule, GeometryReport, check_stability, evaluate_geometry, evaluate_trajectory,  # noqa: F401
                         evaluate_samples)
from .similarity import shape_tanimoto, get_rocs, esp_similarity, align_shapes, similarity_to_condition  # noqa: F401
from .mol_graph import GraphReport, bond_graph, bond_graph_trajectory, bond_graph_samples, atom_type_jsd, to_molblock  # noqa: F401

__version__ = "0.3.0"
