#!/bin/bash
# timing of mcba_observation_covariance at 8 x 500 x 2 (cfg3) and 16 x 1000 x 5 (cfg4): profiles/obs_cov_timing.txt
set -o pipefail
OUT=${1:-profiles/obs_cov_timing.txt}
timeout -k 10 300 python profiles/scripts/prof_obs_cov.py cfg3 2>&1 | tee "$OUT" &&
timeout -k 10 420 python profiles/scripts/prof_obs_cov.py cfg4 2>&1 | tee -a "$OUT"
