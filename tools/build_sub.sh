#!/bin/bash
# Dev builds: libspx with ONE text substitution applied to a copy of the
# sources (the product source carries no switches) -> tools/bin/libspx_NAME.so
#   tools/build_sub.sh NAME 'old text' 'new text'
set -e
exec python3 "$(dirname "$0")/spx_variant.py" "$1" "$2" "$3"
