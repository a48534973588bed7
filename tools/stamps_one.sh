#!/bin/bash
# tools/stamps_one.sh <lib> <variant> <file> <nchunk> <cpd> <cycles> : one stamped run + table.  The stamped launch of the
# diagnostic build writes <file> (stamps_<tag>.txt, csrc/espnet_diag.inc) into $GS_STAMP_DIR (unset: the working directory);
# the run's log goes beside it.
export GLOMSEG_EXPERIMENT=1 GLOMSEG_ALLOW_DIAG=1 GLOMSEG_LIB=$1
export GS_STAMP_DIR=${GS_STAMP_DIR:-.}
log=$GS_STAMP_DIR/stamps_run_$2.log
GS_VARIANT=$2 timeout -k 10 300 python tools/stamps_run.py > $log 2>&1 || { echo "variant $2 failed"; tail -5 $log; exit 1; }
echo "==== $1 GS_VARIANT=$2"
python tools/stamps3.py $GS_STAMP_DIR/$3 $4 $5 $6
