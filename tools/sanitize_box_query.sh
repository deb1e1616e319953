#!/bin/bash
# The host twins of box queries (mi_box_query_host, mi_box_offsets_host, mi_box_fill_host) under AddressSanitizer +
# UndefinedBehaviorSanitizer:
# tools/sanitize_box_query.c built and run by tools/sanitize_standalone.sh. CPU only; nothing is loaded into python.
#   tools/sanitize_box_query.sh
exec "$(dirname "$0")/sanitize_standalone.sh" box_query
