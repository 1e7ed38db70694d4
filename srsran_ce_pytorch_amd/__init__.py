"""MI355X-native PUSCH DM-RS channel estimator (batched, HIP kernels behind a C ABI)."""
from .config import EstimatorConfig, HopConfig, empty_hop  # noqa: F401
from .channel import PuschChannelEmulator, cfo_word, taps_from_delays  # noqa: F401
from .deprecode import PuschTransformDeprecoder  # noqa: F401
from .dmrs import PuschLowPaprDmrs  # noqa: F401
from .encoder import PuschTransportEncoder  # noqa: F401
from .fronthaul import PuschFronthaulCompressor, PuschFronthaulDecompressor, bfp_pack, bfp_unpack  # noqa: F401
from .ldpc import LdpcGraph, PuschLdpcDecoder  # noqa: F401
from .modulator import PuschModulator  # noqa: F401
from .ofdm import PuschOfdmDemodulator, PuschOfdmModulator  # noqa: F401
from .prach import PrachDetector, prach_arrival_seconds, prach_preamble_freq, prach_root_freq, prach_windows  # noqa: F401
from .precode import PuschTransformPrecoder  # noqa: F401
from .ratematch import PuschRateRecovery, select_base_graph  # noqa: F401
from .srs import SrsEstimate, SrsEstimator, SrsProfile, srs_band_response, srs_map, srs_ports, srs_sequence  # noqa: F401
from .transportblock import PuschTransportBlock  # noqa: F401
