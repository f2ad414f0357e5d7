"""Minimal ``DynConfig``: exactly the keys the dense prediction path reads ("Config / flags").

Mirrors /root/reference/syconn/handler/config.py:
* YAML ``config.yml`` in the working directory overlaid on package defaults (``__getitem__`` fallback, :201-215);
* working directory taken from env ``syconn_wd`` (set for worker processes, batchjob_utils.py:223) or from
  ``global_params.wd``, re-checked on every access (``_check_actuality``, :238-267);
* model paths ``mpath_*`` (:613-656), ``kd_seg_path`` (:294-299), ``ngpu_total`` (:799-801).
Geometry (chunk / tile / halo) is additionally exposed under ``dense_prediction`` -- the reference hard-codes it
with a "TODO: these should be config parameters" (prediction.py:671-677).
"""
import logging
import os
from typing import Dict, Any, Optional

import yaml

DEFAULTS = {
    'scaling': [1, 1, 1],
    'batch_proc_system': None,        # the SLURM machinery is out of scope: local one-process-per-GPU launcher
    'ncores_per_node': os.cpu_count() or 8,
    'ngpus_per_node': 8,              # one MI355X node
    'nnodes_total': 1,
    'log_level': 20,
    'default_log_dir': None,
    'disable_file_logging': True,
    'paths': {'kd_seg': None, 'kd_sj': None, 'kd_sym': None, 'kd_asym': None},
    # synapse-type datasets (config.py:700-707): False = no sym / asym masks (cs_extraction_steps.py:431-433)
    'syntype_avail': False,
    'process_cell_organelles': ['mi', 'vc'],      # config.yml:15
    # cells from the supervoxel graph (config.yml:60): components whose bounding box diagonal (nm) is not above this are dropped
    'min_cc_size_ssv': 5000,
    'dense_prediction': {
        'overlap_shape_tiles': [30, 31, 20],   # xyz, prediction.py:672
        'chunk_size': [482, 481, 236],         # prediction.py:674
        'tile_shape': [271, 181, 138],         # prediction.py:677
        # storage type of the activations on the device.  'f16x2' = the reference's precision (it computes in fp32,
        # prediction.py:777-779) on the matrix cores; the fast plans 'f16' / 'bf16' (~3.4x the throughput, 0.06 % / 0.45 % of
        # the threshold-rule labels differ from fp32) are an explicit choice; 'f32' = fp32 FMA arithmetic, ~30x slower
        'act_dtype': 'f16x2',
        # model tiles whose whole result lies beyond the dataset boundary are not predicted (the reference's chunk grid covers
        # up to 1.9x the dataset and it predicts all of it); False reproduces the reference's values in that overhang too
        'skip_tiles_outside_dataset': True,
        # model tiles that reach beyond the dataset boundary are predicted on the part of their window the voxels inside the
        # dataset depend on (identical values there; GroupNorm networks always use full windows)
        'clip_boundary_tiles': True,
        # fp16 range guard: a chunk whose activations overflow fp16 storage is predicted again in the plan with fp32's exponent range
        # ('f16x2' -> 'f32', 'f16' -> 'bf16'); False = only that chunk, True = the worker stays in the fallback plan for its remaining chunks
        'sticky_overflow_fallback': False,
    },
    # first consumer of the probability maps (object extraction): the reference's defaults,
    # /root/reference/syconn/handler/config.yml:108-136
    'cell_objects': {
        'probathresholds': {'mi': 0.428571429, 'sj': 0.19047619, 'vc': 0.285714286, 'er': 0.5, 'golgi': 0.5},
        'min_seed_vx': {'mi': 50, 'sj': 10, 'vc': 10, 'er': 30, 'golgi': 30},
        # size threshold applied during object extraction (config.yml:80-89); sv: all cell supervoxels are extracted
        'min_obj_vx': {'mi': 500, 'sj': 100, 'vc': 100, 'er': 100, 'golgi': 100, 'sv': 1, 'cs': 10, 'syn': 10, 'syn_ssv': 100},
        'extract_morph_op': {
            'mi': ['binary_opening', 'binary_closing', 'binary_erosion', 'binary_erosion', 'binary_erosion', 'binary_erosion'],
            'sj': ['binary_opening', 'binary_closing', 'binary_erosion'],
            'vc': ['binary_opening', 'binary_closing', 'binary_erosion'],
            'er': ['binary_dilation'] * 3 + ['binary_erosion'] * 3,
            'golgi': ['binary_dilation'] * 3 + ['binary_erosion'] * 3,
        },
        # contact sites (config.yml:146-150): the stencil of the partner search (odd extents; max // 2 closings follow) and the
        # dilations after the closing
        'cs_filtersize': [13, 13, 7],
        'cs_dilation': 2,
        # labels of the synapse types in the kd_sym / kd_asym segmentations (config.py:803-809); None: those datasets hold raw
        # data, thresholded at 123 (cs_extraction_steps.py:414-424)
        'sym_label': None,
        'asym_label': None,
        # synapse agglomeration (config.yml:152, :164): fragments of one cell pair closer than cs_gap_nm form one syn_ssv object;
        # a symmetric ratio above sym_thresh gives syn_sign -1
        'cs_gap_nm': 250,
        'sym_thresh': 0.225,
        # organelles mapped to the cell-level synapses (config.yml:156-159): a mesh vertex closer than max_vert_dist_nm to a synapse
        # voxel counts as close; organelles whose representative coordinate is farther than max_rep_coord_dist_nm are not looked at
        'max_vert_dist_nm': {'mi': 1000, 'vc': 500},
        'max_rep_coord_dist_nm': 4000,
        # export_matrix(threshold_syn=None) keeps the synapses with a probability above this (config.yml:161)
        'thresh_synssv_proba': 0.5,
        # organelles to cells (config.yml:92-106): an organelle belongs to a cell that holds more than the lower and at most the upper
        # share of its voxels (an upper ratio of 1 or more is not tested) if it has more voxels than the size threshold
        'lower_mapping_ratios': {'mi': 0.5, 'sj': 0.1, 'vc': 0.5},
        'upper_mapping_ratios': {'mi': 1., 'sj': 0.9, 'vc': 1.},
        'sizethresholds': {'mi': 2786, 'sj': 498, 'vc': 1584},
    },
    # partner properties of the cell-level synapses (config.yml:271-274, :278, :288, :303): the vote over the k nearest mesh vertices
    # (every ds_vertices-th one, without the ignored labels), the skeleton key of the compartment, the length of the embedding
    'spines': {'semseg2coords_spines': {'k': 50, 'ds_vertices': 1, 'ignore_labels': [4, 5]},
               # semseg2mesh of the spine labels (config.yml:265-267): k = 0 keeps unpredicted vertices as their own class
               'semseg2mesh_spines': {'semseg_key': 'spiness', 'k': 0}},
    # compartment views and the mapping of their vertex labels to skeleton nodes (config.yml:283-295)
    'compartments': {'dist_axoness_averaging': 10000,
                     'view_properties_semsegax': {'verbose': False, 'ws': [1024, 512], 'nb_views': 3, 'comp_window': 40960, 'semseg_key': 'axoness',
                                                  'k': 0},
                     'map_properties_semsegax': {'k': 50, 'ds_vertices': 1, 'ignore_labels': [5, 6]}},
    'tcmn': {'ndim_embedding': 10},
    # surface meshes (config.yml:169-189): the downsampling of every label volume before meshing, the size below which an object keeps
    # an empty mesh, and the arguments of zmesh's get_mesh -- the two simplification keys are accepted and IGNORED (proc/meshes.py
    # builds the unsimplified surface), normals: True is not built
    'meshes': {
        'allow_mesh_gen_cells': False,
        'use_new_meshing': True,
        'downsampling': {'sv': [4, 4, 2], 'sj': [2, 2, 1], 'vc': [4, 4, 2], 'mi': [4, 4, 2], 'er': [2, 2, 1], 'golgi': [2, 2, 1]},
        'mesh_min_obj_vx': 100,
        'meshing_props': {'normals': False, 'simplification_factor': 50, 'max_simplification_error': 40},
    },
    # astrocyte splitting (config.yml:221, :243-247): run before the neuron cells are made; a supervoxel is glia when the mean of its
    # views' glia probability is above glia_thresh and more than 70 % of the views are (point models: the mean at or above it)
    'glia': {'prior_astrocyte_removal': True, 'glia_thresh': 0.161489},
    'use_point_models': False,
    # views (config.yml:223-232): the organelle channels after the cell's ('sj' is rendered from 'syn_ssv' with on-the-fly views), the
    # window edge in nm along the first principal axis, the window in pixels (x, y) and the views per location; the rule of the rendering
    # locations (config.yml:225): generate_rendering_locs, else the legacy surface_samples
    'views': {
        'use_onthefly_views': True,
        'use_new_renderings_locs': True,
        'subcell_objects': ['mi', 'vc', 'sj'],
        'view_properties': {'comp_window': 8000, 'ws': [256, 128], 'nb_views': 2},
    },
    # cell types from multi-views (config.yml:297-299): the views per sample of the view network
    'celltypes': {'nb_views_model': 20},
    # skeletons from the label volume (config.yml:211); False selects the mesh-based fallback, which is not built
    'use_kimimaro': True,
}


class DynConfig:
    def __init__(self, wd: Optional[str] = None):
        self._wd = None
        self._entries = {}
        self.initialized = False
        if wd is not None:
            self._load(wd)

    def _load(self, wd: str):
        self._wd = os.path.abspath(os.path.expanduser(wd))
        self._entries = {}
        p = self.path_config
        self.initialized = os.path.isfile(p)
        if self.initialized:
            with open(p) as f:
                self._entries = yaml.safe_load(f) or {}

    def _check_actuality(self):
        from .. import global_params
        new_wd = None
        env = os.environ.get('syconn_wd')
        if env and env != 'None':
            if self._wd != os.path.abspath(os.path.expanduser(env)):
                new_wd = env
        elif global_params.wd and global_params.wd != 'None' and \
                self._wd != os.path.abspath(os.path.expanduser(global_params.wd)):
            new_wd = global_params.wd
        if new_wd is not None:
            self._load(new_wd)

    @property
    def path_config(self) -> str:
        return f'{self._wd}/config.yml'

    @property
    def working_dir(self) -> str:
        self._check_actuality()
        if self._wd is None:
            raise ValueError('working directory not set (global_params.wd or env syconn_wd)')
        return self._wd

    def __getitem__(self, item: str) -> Any:
        self._check_actuality()
        if item in self._entries and self._entries[item] is not None:
            v = self._entries[item]
            if isinstance(v, dict) and isinstance(DEFAULTS.get(item), dict):
                merged = dict(DEFAULTS[item])
                merged.update({k: x for k, x in v.items() if x is not None})
                return merged
            return v
        if item in DEFAULTS:
            return DEFAULTS[item]
        raise KeyError(item)

    @property
    def kd_seg_path(self) -> str:
        return self['paths']['kd_seg']

    def __getattr__(self, name: str):
        # kd_<name>_path (config.py:300-360: kd_sym / kd_asym / kd_sj / kd_vc / kd_mi / kd_er / kd_golgi): the probability-map datasets
        if name.startswith('kd_') and name.endswith('_path') and name != 'kd_seg_path':
            key = name[:-len('_path')]
            try:
                return self['paths'][key]
            except KeyError:
                raise AttributeError(f"config['paths'] has no '{key}'") from None
        raise AttributeError(name)

    @property
    def kd_organelles_paths(self) -> Dict[str, str]:
        """config.py:362-373: probability-map KnossosDatasets of ``config['process_cell_organelles']``."""
        return {k: self['paths']['kd_{}'.format(k)] for k in self['process_cell_organelles']}

    @property
    def kd_organelle_seg_paths(self) -> Dict[str, str]:
        """config.py:375-386: where the organelle SEGMENTATION KnossosDatasets live."""
        return {k: "{}/knossosdatasets/{}_seg/".format(self.working_dir, k) for k in self['process_cell_organelles']}

    @property
    def temp_path(self) -> str:
        return "{}/tmp/".format(self.working_dir)

    @property
    def model_dir(self) -> str:
        return self.working_dir + '/models/'

    @property
    def mpath_myelin(self) -> str:
        return self.model_dir + '/myelin/model.pts'

    @property
    def mpath_syntype(self) -> str:
        return self.model_dir + '/syntype/model.pts'

    @property
    def mpath_er(self) -> str:
        return self.model_dir + '/er/model.pts'

    @property
    def mpath_golgi(self) -> str:
        return self.model_dir + '/golgi/model.pts'

    @property
    def mpath_mivcsj(self) -> str:
        return self.model_dir + '/mivcsj/model.pt'

    @property
    def mpath_glia_e3(self) -> str:
        """config.py:594-600: the view network that tells glia from neuron supervoxels.  The reference names the model's folder; the
        file in it is ``model.pts`` as for the other view networks."""
        return self.model_dir + '/glia_e3/model.pts'

    @property
    def mpath_celltype_e3(self) -> str:
        """config.py:565-570: the view network of the cell type step."""
        return self.model_dir + '/celltype_e3/model.pts'

    @property
    def mpath_tnet(self) -> str:
        """config.py:485-492: the encoder of local cell morphology trained with a triplet loss (tCMN)."""
        return self.model_dir + '/tCMN/model.pts'

    @property
    def mpath_spiness(self) -> str:
        """config.py:537-544: the 2D semantic-segmentation model of spine head, neck, shaft and other."""
        return self.model_dir + '/spiness/model.pts'

    @property
    def mpath_axonsem(self) -> str:
        """config.py:546-553: the 2D semantic-segmentation model of axon, boutons, dendrite and soma."""
        return self.model_dir + '/axoness_semseg/model.pts'

    @property
    def syntype_available(self) -> bool:
        """config.py:700-708: synaptic types are available as KnossosDataset(s)."""
        return bool(self['syntype_avail'])

    @property
    def asym_label(self) -> Optional[int]:
        return self['cell_objects']['asym_label']

    @property
    def sym_label(self) -> Optional[int]:
        return self['cell_objects']['sym_label']

    @property
    def ncore_total(self) -> int:
        """config.py:795-797."""
        return self['nnodes_total'] * self['ncores_per_node']

    @property
    def ngpu_total(self) -> int:
        return self['nnodes_total'] * self['ngpus_per_node']


def generate_default_conf(working_dir: str, scaling=(1, 1, 1), kd_seg: Optional[str] = None,
                          key_value_pairs=None):
    """Write ``<wd>/config.yml`` (reference: config.py:812-931, reduced to this path's keys)."""
    os.makedirs(working_dir, exist_ok=True)
    entries = {'scaling': list(scaling), 'paths': {'kd_seg': kd_seg}}
    for k, v in (key_value_pairs or []):
        entries[k] = v
    with open(f'{working_dir}/config.yml', 'w') as f:
        yaml.safe_dump(entries, f)


def initialize_logging(log_name: str, log_dir: Optional[str] = None, overwrite: bool = True) -> logging.Logger:
    """Logger factory (reference: config.py:934-995); std logging instead of coloredlogs."""
    from .. import global_params
    logger = logging.getLogger(log_name)
    try:
        level = global_params.config['log_level']
    except (KeyError, ValueError):
        level = logging.INFO
    logger.setLevel(level)
    if not logger.handlers:
        sh = logging.StreamHandler()
        sh.setFormatter(logging.Formatter('%(asctime)s [%(name)s] %(levelname)s: %(message)s'))
        logger.addHandler(sh)
    if log_dir is not None:
        os.makedirs(log_dir, exist_ok=True)
        fp = os.path.join(log_dir, log_name + '.log')
        if overwrite and os.path.isfile(fp):
            os.remove(fp)
        if not any(isinstance(h, logging.FileHandler) and h.baseFilename == os.path.abspath(fp)
                   for h in logger.handlers):
            fh = logging.FileHandler(fp)
            fh.setFormatter(logging.Formatter('%(asctime)s [%(name)s] %(levelname)s: %(message)s'))
            logger.addHandler(fh)
    return logger
