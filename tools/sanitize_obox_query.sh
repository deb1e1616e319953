#!/bin/bash
# The host twins of oriented-box queries (mi_obox_query_host, mi_obox_offsets_host, mi_obox_fill_host) under AddressSanitizer +
# UndefinedBehaviorSanitizer:
# tools/sanitize_obox_query.c built and run by tools/sanitize_standalone.sh. CPU only; nothing is loaded into python.
#   tools/sanitize_obox_query.sh
exec "$(dirname "$0")/sanitize_standalone.sh" obox_query
