"""descriptools_amd -- MI355X-native drop-in for the descriptools terrain-descriptor hot path.

Same module / function names as the reference package (callers import the submodules, as
Example/example.py:11-16 does): slope, flowhand, topoindexes, gfi, downslope, evaluation, helpers;
net-new: flowdir (D8), flowacc, streams (stream order and links), watershed (basins, flow lengths), reaches (reach
catchments, stage tables, rating curves, inundation), dinf (D-infinity direction and contributing area), mfd
(multiple-flow-direction shares and contributing area), routing (decayed, retention- and transport-limited
accumulation on those flow fields: fill and spill, run-on losses), proximity (Euclidean nearest-river distance, allocation and
HAND), regions (connected regions of a mask: labels, sizes, river-connected and sieved flood extents), chain
(device-resident full chain), tiling (multi-GPU).
All compute goes through libdescriptools_hip.so (include/descriptools_hip.h); there is no CPU path.
"""
__version__ = "0.1.0"
