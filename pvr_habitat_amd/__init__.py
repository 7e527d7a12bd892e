"""pvr_habitat_amd: MI355X-native PVR embedding + behavioural-cloning hot path.

Python host side mirrors the reference call surface (sparisi/pvr_habitat src/embeddings.py,
src/models.py, behavioral_cloning/save_embedded_obs.py, main_bc_*.py); the arithmetic lives in
hand-written HIP kernels behind the C-ABI of include/pvr_hip.h (libpvr_hip.so).
"""
# The ROCm runtime multiplexes HIP streams onto a few hardware queues.  This package keeps five streams busy (torch's current stream,
# two compute lanes, H2D, D2H); when they share queues the copy streams serialise with the lanes - stream_embed ran at 53 k frames/s
# with four queues and 75 k with eight inside bench.py (profiles/experiments/r02_stream_creation_order.txt).  The package does not
# change the queue count: it runs with whatever the environment gives the process.

__version__ = '0.1.0'
