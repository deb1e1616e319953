#!/bin/bash
# The host twins of frustum queries (mi_frustum_query_host, mi_frustum_offsets_host, mi_frustum_fill_host) under AddressSanitizer +
# UndefinedBehaviorSanitizer:
# tools/sanitize_frustum_query.c built and run by tools/sanitize_standalone.sh. CPU only; nothing is loaded into python.
#   tools/sanitize_frustum_query.sh
exec "$(dirname "$0")/sanitize_standalone.sh" frustum_query
