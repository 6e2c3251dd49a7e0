"""HIP-backed mirrors of the reference's L1 modules (same constructor arguments, method names, dict keys, state-dict
keys and error behaviour).  GenericTrainer / Runner of the reference can use them unchanged."""
from .sparse_sdf_network import SparseSdfNetwork, LatentSDFLayer  # noqa: F401
from .rendering_network import GeneralRenderingNetwork  # noqa: F401
from .sparse_neus_renderer import SparseNeuSRenderer, Projector  # noqa: F401
from .fields import SingleVarianceNetwork  # noqa: F401
from .packs import pack_stats  # noqa: F401
