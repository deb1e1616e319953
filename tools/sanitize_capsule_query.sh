#!/bin/bash
# The host twins of capsule queries (mi_capsule_query_host, mi_capsule_offsets_host, mi_capsule_fill_host) under AddressSanitizer +
# UndefinedBehaviorSanitizer:
# tools/sanitize_capsule_query.c built and run by tools/sanitize_standalone.sh. CPU only; nothing is loaded into python.
#   tools/sanitize_capsule_query.sh
exec "$(dirname "$0")/sanitize_standalone.sh" capsule_query
