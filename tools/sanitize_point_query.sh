#!/bin/bash
# The host twin of point queries (mi_point_query_host) under AddressSanitizer + UndefinedBehaviorSanitizer:
# tools/sanitize_point_query.c built and run by tools/sanitize_standalone.sh. CPU only; nothing is loaded into python.
#   tools/sanitize_point_query.sh
exec "$(dirname "$0")/sanitize_standalone.sh" point_query
