#!/bin/bash
# Build libpadel_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU).
set -e
cd "$(dirname "$0")"
# PADEL_EXTRA_FLAGS=-DPADEL_RENDER_PROBE clocks render.hip's cull and apply phases inside the kernel and reports them per call on
# stderr (profiles/render_bench.txt; right results); PADEL_OUT / PADEL_BUILD_DIR keep such a build apart from the product library
# (tools only).  No flag builds a kernel that computes wrong results any more
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -Wno-unused-value ${PADEL_EXTRA_FLAGS:-}"
BUILD="${PADEL_BUILD_DIR:-build}"
OUT="${PADEL_OUT:-../libpadel_hip.so}"
mkdir -p "$BUILD"
pids=()
# PADEL_ONLY="a.hip b.hip": recompile only these translation units and relink with the objects already in $BUILD (iteration)
ALL="conv_tap.hip conv_tap16.hip conv_tap_bx3.hip conv_patch_bx3.hip conv_tap_h2.hip conv_tap_h2p.hip conv_1x1_h2s.hip conv_patch_h2.hip conv_patch_h2q.hip conv_patch_h2r.hip conv_patch_h2v.hip conv_patch_h2w.hip conv_patch16.hip kernels_misc.hip resnet_ops.hip yolo11_ops.hip stem_l1_h2.hip head_tail_h2.hip postproc.hip tracknet_post.hip yuv_convert.hip render.hip jpeg_encode.hip jpeg_decode.hip frame_activity.hip box_histogram.hip warp.hip heat.hip"
# the engine (host code that calls the HIP runtime), one translation unit per concern: engine_internal.h
ENGINE="engine.cpp engine_pre.cpp engine_yolo.cpp engine_tracknet.cpp engine_resnet.cpp engine_comm.cpp engine_render.cpp engine_jpeg.cpp engine_jpeg_decode.cpp engine_activity.cpp engine_warp.cpp engine_heat.cpp"
for f in ${PADEL_ONLY:-$ALL $ENGINE}; do
  [ -f "$f" ] || continue
  # per-file flags.  warp.hip: its doubles are pinned bit for bit against the host (warp_math.h), and at -O3 the _rn intrinsics
  # do not keep hipcc from fusing a multiply into an add and a contract pragma was not dependable; the command-line flag is
  case "$f" in
    warp.hip) EXTRA="-ffp-contract=off" ;;
    *) EXTRA="" ;;
  esac
  case "$f" in
    *.cpp) hipcc $FLAGS $EXTRA -x hip -c "$f" -o "$BUILD/${f%.cpp}.o" & ;;
    *) hipcc $FLAGS $EXTRA -c "$f" -o "$BUILD/${f%.hip}.o" & ;;
  esac
  pids+=($!)
done
# host code; -ffp-contract=off: the tracker's doubles are pinned against the Python twin (no fused multiply-adds)
if [ -z "${PADEL_ONLY:-}" ]; then
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -c bytetrack.cpp -o "$BUILD/bytetrack.o" &
pids+=($!)
# which kernel runs a conv (tile table, resolver, choosers): no HIP runtime call, only the types of kernels.h
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include ${PADEL_EXTRA_FLAGS:-} -c conv_select.cpp -o "$BUILD/conv_select.o" &
pids+=($!)
# what is decided about a graph before anything runs (refusals, upsample folds, memory plan, resize tables): no HIP runtime call either
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include ${PADEL_EXTRA_FLAGS:-} -c graph_plan.cpp -o "$BUILD/graph_plan.o" &
pids+=($!)
# what one replay of an op list launches, and with which arguments: no HIP runtime call either
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include ${PADEL_EXTRA_FLAGS:-} -c launch_plan.cpp -o "$BUILD/launch_plan.o" &
pids+=($!)
# what pa_render refuses, and the font: no HIP at all (the same file builds into tests/render_marks_main.cpp's program)
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -c render_check.cpp -o "$BUILD/render_check.o" &
pids+=($!)
# what pa_warp_perspective refuses: no HIP at all (the same file builds into tests/warp_main.cpp's program)
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -c warp_check.cpp -o "$BUILD/warp_check.o" &
pids+=($!)
# what pa_heat_accumulate refuses: no HIP at all (heat_math.h also builds into tests/heat_main.cpp's program)
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -c heat_check.cpp -o "$BUILD/heat_check.o" &
pids+=($!)
# what pa_frame_activity refuses, and how a launch is cut into bands: no HIP at all (the same file builds into tests/activity_check_main.cpp's program)
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -c activity_check.cpp -o "$BUILD/activity_check.o" &
pids+=($!)
# what pa_box_histograms refuses: no HIP at all (the same file builds into tests/box_histogram_check_main.cpp's program)
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -c box_histogram_check.cpp -o "$BUILD/box_histogram_check.o" &
pids+=($!)
# what pa_jpeg_encode refuses, its tables, header and sizes: no HIP either (jpeg_tables.h also builds into tests/jpeg_tables_main.cpp's program)
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -c jpeg_check.cpp -o "$BUILD/jpeg_check.o" &
pids+=($!)
# the markers of a JPEG that pa_jpeg_decode reads, and pa_jpeg_parse: no HIP either (the same file builds into tests/jpeg_decode_main.cpp's program)
g++ -O3 -ffp-contract=off -std=c++17 -fPIC -Wall -c jpeg_parse.cpp -o "$BUILD/jpeg_parse.o" &
pids+=($!)
fi
for p in "${pids[@]}"; do wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" "$BUILD"/*.o -Wl,-rpath,/opt/rocm/lib
echo "built $OUT"
