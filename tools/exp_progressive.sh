#!/bin/bash
# The progressive reader against starting over, 512^3 f32 (tools/exp_progressive.py): each GPU step under
# its own time limit, nothing started after one that failed.
set -o pipefail
cd "$(dirname "$0")/.."
timeout -k 10 120 python tools/exp_progressive.py 128 3 &&
timeout -k 10 400 python tools/exp_progressive.py 512 7
