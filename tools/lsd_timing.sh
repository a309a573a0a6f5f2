#!/bin/bash
# rebuild the line extractor (lsd_*.hip) with -DPLF_LSD_TIMING into a scratch library, where tools/lsd_timing*.py look for it (PLF_TIMING_LIB); they print the
# per-section cycle counts (frame 0).  PLF_TIMING_EXTRA: further flags for the same files, e.g. -DPLF_LSD_TIMING_NOCNT (cycles without the counters' global
# read-modify-writes) or -DPLF_TIMING_BAND=5 (which band wave is timed)
set -e
bash "$(dirname "$0")/variant_build.sh" timing "lsd_*.hip=-DPLF_LSD_TIMING $PLF_TIMING_EXTRA"
mkdir -p /tmp/plft && cp "$(dirname "$0")/scratch/libplf_timing.so" /tmp/plft/libplf_hip.so
