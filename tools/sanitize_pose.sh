#!/bin/bash
# The host twin of rigid poses (mi_pose_geometry_host) under AddressSanitizer + UndefinedBehaviorSanitizer:
# tools/sanitize_pose.c built and run by tools/sanitize_standalone.sh. CPU only; nothing is loaded into python.
#   tools/sanitize_pose.sh
exec "$(dirname "$0")/sanitize_standalone.sh" pose
