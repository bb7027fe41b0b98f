# Build recipe (no cmake needed): product library (HIP, gfx950), synthetic-frame helper (C),
# and the CPU oracle (C++, test infrastructure).  `python -c "import __graft_entry__ as g; g.build()"` runs this.
HIPCC      ?= /opt/rocm/bin/hipcc
CXX        ?= g++
CC         ?= gcc
ARCH       ?= gfx950
# -amdgpu-mfma-vgpr-form: the matcher's MFMA results feed VALU min / compare trees, so they should land in VGPRs (no v_accvgpr_read per value)
HIPFLAGS   := --offload-arch=$(ARCH) -O3 -std=c++20 -fPIC -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form -Wall -Wno-unused-function -Iinclude -Iorb_slam_amd/csrc
ORBX_SRCS  := $(wildcard orb_slam_amd/csrc/*.hip)
ORBX_HDRS  := $(wildcard orb_slam_amd/csrc/*.h orb_slam_amd/csrc/*.inc include/*.h)

all: orb_slam_amd/liborbx.so orb_slam_amd/libsynthframes.so oracle/liborb_oracle.so oracle_ref orb_slam_amd/cpp/example_frame orb_slam_amd/cpp/example_batch orb_slam_amd/cpp/example_color orb_slam_amd/cpp/example_pipeline orb_slam_amd/cpp/example_lanes orb_slam_amd/cpp/bench_single_frame tests/kfdb_dropin/harness tests/mappoints_dropin/harness tests/source_dropin/harness tests/triangulate_dropin/harness tests/refresh_dropin/harness tests/fuse_dropin/harness tests/loop_dropin/harness tests/sim3_dropin/harness tests/bow_dropin/harness tests/newpoints_dropin/harness tests/localmap_dropin/harness tests/cull_dropin/harness tests/init_dropin/harness tests/init_dropin/harness_host tests/pnp_dropin/harness tests/pnp_dropin/harness_host tools/libmappoints_host.so tools/liblocalmap_host.so tools/libcull_host.so tools/libsource_host.so tools/libtriangulate_host.so tools/librefresh_host.so tools/libfuse_host.so tools/libloop_host.so tools/libsim3_host.so tools/libinit_host.so tools/libpnp_host.so tools/microbench/valu_rate tools/microbench/valu_rate2 tools/microbench/mfma_layout tools/microbench/mfma_layout_fp4 tools/microbench/mfma_valu_mix tools/microbench/fetch_calib tools/microbench/valu_exec_mask tools/microbench/ta_shapes

# the hash of the kernel sources travels inside the library (orbx_build_id): counters replayed by bench.py must come from THIS build
SRC_HASH   := $(shell cat $(sort $(ORBX_SRCS) $(ORBX_HDRS)) | sha256sum | cut -c1-16)
# one object per translation unit (round 6: the extractor's kernels are split by stage; `make -j` compiles them side by side).  The hash goes into
# the one file that reports it, which therefore depends on every source.
OBJDIR     := build/orbx
ORBX_OBJS  := $(patsubst orb_slam_amd/csrc/%.hip,$(OBJDIR)/%.o,$(ORBX_SRCS))
$(OBJDIR)/%.o: orb_slam_amd/csrc/%.hip $(ORBX_HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJDIR)/orbx_api.o: orb_slam_amd/csrc/orbx_api.hip $(ORBX_SRCS) $(ORBX_HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -DORBX_SRC_HASH='"$(SRC_HASH)"' -c $< -o $@
orb_slam_amd/liborbx.so: $(ORBX_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared $(ORBX_OBJS) -o $@

orb_slam_amd/libsynthframes.so: orb_slam_amd/csrc/synth_frames.c
	$(CC) -O2 -fPIC -shared $< -o $@

# oracle: scalar restatement, ISO float evaluation (no FMA contraction), the CPU baseline build flags of SURVEY §8d
oracle/liborb_oracle.so: oracle/orb_oracle.cpp oracle/bow_oracle.cpp oracle/frame_oracle.cpp oracle/search_oracle.cpp oracle/orb_pattern_points.inc
	$(MAKE) -C oracle liborb_oracle.so

# the reference's own sources compiled against stand-in cv headers (only where /root/reference exists): oracle/Makefile
oracle_ref: oracle/liborb_oracle.so orb_slam_amd/liborbx.so
	$(MAKE) -C oracle ref

# C++ shim demo: the reference's Frame-side call sequence against the drop-in classes (host C++, links the C ABI)
orb_slam_amd/cpp/example_frame: orb_slam_amd/cpp/example_frame.cpp orb_slam_amd/cpp/ORBextractor.h orb_slam_amd/cpp/ORBmatcher.h orb_slam_amd/cpp/ORBVocabulary.h orb_slam_amd/cpp/cvcompat.h include/orbx.h include/orbv.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Iinclude -Iorb_slam_amd/cpp $< -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib

# several host frames in one call (ORBextractor::ExtractBatch over orbx_extract_batch), checked against the one-frame call
orb_slam_amd/cpp/example_batch: orb_slam_amd/cpp/example_batch.cpp orb_slam_amd/cpp/ORBextractor.h orb_slam_amd/cpp/cvcompat.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Iinclude -Iorb_slam_amd/cpp $< -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib

# colour frames: ORBextractor::GrabImage (Tracking::GrabImage + Frame::Frame) and the colour ExtractBatch, checked against the gray operator()
orb_slam_amd/cpp/example_color: orb_slam_amd/cpp/example_color.cpp orb_slam_amd/cpp/ORBextractor.h orb_slam_amd/cpp/cvcompat.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Iinclude -Iorb_slam_amd/cpp $< -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib

# the device-resident front-end driven from plain C++ through the C ABI (no HIP headers on the host side)
orb_slam_amd/cpp/example_pipeline: orb_slam_amd/cpp/example_pipeline.cpp include/orbx.h include/orbf.h include/orbv.h include/orbs.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Iinclude $< -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib

# the lanes configuration (LanePipeline.h) from plain C++
orb_slam_amd/cpp/example_lanes: orb_slam_amd/cpp/example_lanes.cpp orb_slam_amd/cpp/LanePipeline.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Iinclude -Iorb_slam_amd/cpp $< -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib

# the drop-in call's latency from plain C++
orb_slam_amd/cpp/bench_single_frame: orb_slam_amd/cpp/bench_single_frame.cpp include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Iinclude $< -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib

# the KeyFrameDatabase drop-in (orb_slam_amd/cpp/KeyFrameDatabase.cc) over stand-in KeyFrame.h / Frame.h, driven by scripts
# (tests/test_gpu_kfdb_dropin.py)
KFDB_DROPIN := orb_slam_amd/cpp/KeyFrameDatabase.cc orb_slam_amd/cpp/KeyFrameDatabase.h orb_slam_amd/cpp/ORBVocabulary.h tests/kfdb_dropin/KeyFrame.h tests/kfdb_dropin/Frame.h
tests/kfdb_dropin/harness: tests/kfdb_dropin/harness.cpp $(KFDB_DROPIN) include/orbd.h include/orbv.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -pthread -Itests/kfdb_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/KeyFrameDatabase.cc -o $@ -Lorb_slam_amd -lorbx \
	    -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# the LocalMapPoints drop-in (orb_slam_amd/cpp/LocalMapPoints.cc) over stand-in Frame.h / MapPoint.h, driven by scripts
# (tests/test_gpu_mappoints_dropin.py)
MP_DROPIN := orb_slam_amd/cpp/LocalMapPoints.cc orb_slam_amd/cpp/LocalMapPoints.h orb_slam_amd/cpp/ORBmatcherAccess.h $(wildcard tests/mappoints_dropin/*.h)
tests/mappoints_dropin/harness: tests/mappoints_dropin/harness.cpp $(MP_DROPIN) include/orbp.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/LocalMapPoints.cc -o $@ -Lorb_slam_amd -lorbx \
	    -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# the last-frame / key-frame searches of the drop-in (orb_slam_amd/cpp/LocalMapPointsSource.cc) over stand-in Frame.h / KeyFrame.h, driven by
# scripts (tests/test_gpu_source_dropin.py); MapPoint.h and cvmini.h are those of tests/mappoints_dropin
SRC_DROPIN := orb_slam_amd/cpp/LocalMapPointsSource.cc $(MP_DROPIN) $(wildcard tests/source_dropin/*.h)
tests/source_dropin/harness: tests/source_dropin/harness.cpp $(SRC_DROPIN) include/orbp.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/source_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/LocalMapPoints.cc \
	    orb_slam_amd/cpp/LocalMapPointsSource.cc -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# LocalMapPoints::Refresh (orb_slam_amd/cpp/LocalMapPointsRefresh.cc) over stand-in MapPoint.h / KeyFrame.h, driven by scripts
# (tests/test_gpu_refresh_dropin.py); Frame.h and cvmini.h are those of tests/mappoints_dropin
RF_DROPIN := orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPoints.cc orb_slam_amd/cpp/LocalMapPoints.h orb_slam_amd/cpp/ORBmatcherAccess.h \
    $(wildcard tests/refresh_dropin/*.h) tests/mappoints_dropin/Frame.h tests/mappoints_dropin/cvmini.h
tests/refresh_dropin/harness: tests/refresh_dropin/harness.cpp $(RF_DROPIN) include/orbp.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/refresh_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/LocalMapPoints.cc \
	    orb_slam_amd/cpp/LocalMapPointsRefresh.cc -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# LocalMapPoints::Fuse / FuseInNeighbors (orb_slam_amd/cpp/LocalMapPointsFuse.cc, over the key-frame store of LocalMapPointsRefresh.cc) over stand-in
# MapPoint.h / KeyFrame.h, driven by scripts (tests/test_gpu_fuse_dropin.py); Frame.h and cvmini.h are those of tests/mappoints_dropin
FU_DROPIN := orb_slam_amd/cpp/LocalMapPointsFuse.cc orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPoints.cc orb_slam_amd/cpp/LocalMapPoints.h \
    orb_slam_amd/cpp/ORBmatcherAccess.h $(wildcard tests/fuse_dropin/*.h) tests/mappoints_dropin/Frame.h tests/mappoints_dropin/cvmini.h
tests/fuse_dropin/harness: tests/fuse_dropin/harness.cpp $(FU_DROPIN) include/orbp.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/fuse_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/LocalMapPoints.cc \
	    orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPointsFuse.cc -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# LocalMapPoints::SearchByProjection(pKF, Scw, ...) / SearchAndFuse (orb_slam_amd/cpp/LocalMapPointsLoop.cc, over searchFuse of LocalMapPointsFuse.cc and the
# key-frame store of LocalMapPointsRefresh.cc) over a stand-in KeyFrame.h, driven by scripts (tests/test_gpu_loop_dropin.py); MapPoint.h is that of
# tests/fuse_dropin, Frame.h and cvmini.h those of tests/mappoints_dropin
LP_DROPIN := orb_slam_amd/cpp/LocalMapPointsLoop.cc $(FU_DROPIN) $(wildcard tests/loop_dropin/*.h)
tests/loop_dropin/harness: tests/loop_dropin/harness.cpp $(LP_DROPIN) include/orbp.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/loop_dropin -Itests/fuse_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/LocalMapPoints.cc \
	    orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPointsFuse.cc orb_slam_amd/cpp/LocalMapPointsLoop.cc -o $@ -Lorb_slam_amd -lorbx \
	    -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# LocalMapPoints::SearchBySim3 (orb_slam_amd/cpp/LocalMapPointsSim3.cc, over residentForFuse of LocalMapPointsFuse.cc and the key-frame store of
# LocalMapPointsRefresh.cc), driven by scripts (tests/test_gpu_sim3_dropin.py); MapPoint.h is this directory's (it adds GetIndexInKeyFrame), KeyFrame.h
# that of tests/loop_dropin, Frame.h and cvmini.h those of tests/mappoints_dropin
S3_DROPIN := orb_slam_amd/cpp/LocalMapPointsSim3.cc $(FU_DROPIN) $(wildcard tests/sim3_dropin/*.h) tests/loop_dropin/KeyFrame.h
tests/sim3_dropin/harness: tests/sim3_dropin/harness.cpp $(S3_DROPIN) include/orbp.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/sim3_dropin -Itests/loop_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/LocalMapPoints.cc \
	    orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPointsFuse.cc orb_slam_amd/cpp/LocalMapPointsSim3.cc -o $@ -Lorb_slam_amd -lorbx \
	    -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# LocalMapPoints::SearchByBoW (orb_slam_amd/cpp/LocalMapPointsBoW.cc, over residentForFuse of LocalMapPointsFuse.cc and the key-frame store of
# LocalMapPointsRefresh.cc), driven by scripts (tests/test_gpu_bow_dropin.py); KeyFrame.h and Frame.h are this directory's (they add the FeatureVector),
# MapPoint.h that of tests/fuse_dropin, cvmini.h that of tests/mappoints_dropin
BW_DROPIN := orb_slam_amd/cpp/LocalMapPointsBoW.cc orb_slam_amd/cpp/FeatureVectorCSR.h $(FU_DROPIN) $(wildcard tests/bow_dropin/*.h)
tests/bow_dropin/harness: tests/bow_dropin/harness.cpp $(BW_DROPIN) include/orbp.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/bow_dropin -Itests/fuse_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/LocalMapPoints.cc \
	    orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPointsFuse.cc orb_slam_amd/cpp/LocalMapPointsBoW.cc -o $@ -Lorb_slam_amd -lorbx \
	    -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# LocalMapPoints::CreateNewMapPoints (orb_slam_amd/cpp/LocalMapPointsNewPoints.cc, over residentForBoW of LocalMapPointsBoW.cc) next to the loop over
# TriangulateNewMapPoints (orb_slam_amd/cpp/NewMapPoints.cc), driven by scripts (tests/test_gpu_newpoints_dropin.py); KeyFrame.h is this directory's (it
# adds the level tables), Frame.h that of tests/bow_dropin, MapPoint.h that of tests/fuse_dropin, cvmini.h that of tests/mappoints_dropin
NP_DROPIN := orb_slam_amd/cpp/LocalMapPointsNewPoints.cc orb_slam_amd/cpp/NewPointsPacking.h orb_slam_amd/cpp/NewMapPoints.cc orb_slam_amd/cpp/NewMapPoints.h \
    orb_slam_amd/cpp/LocalMapPointsBoW.cc orb_slam_amd/cpp/FeatureVectorCSR.h $(FU_DROPIN) tests/bow_dropin/Frame.h $(wildcard tests/newpoints_dropin/*.h)
tests/newpoints_dropin/harness: tests/newpoints_dropin/harness.cpp $(NP_DROPIN) include/orbt.h include/orbp.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/newpoints_dropin -Itests/bow_dropin -Itests/fuse_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< \
	    orb_slam_amd/cpp/LocalMapPoints.cc orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPointsFuse.cc orb_slam_amd/cpp/LocalMapPointsBoW.cc \
	    orb_slam_amd/cpp/LocalMapPointsNewPoints.cc orb_slam_amd/cpp/NewMapPoints.cc -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# LocalMapPoints::PutKeyFrame / UpdateReferenceKeyFrames / SearchLocalMap / ConnectionWeights (orb_slam_amd/cpp/LocalMapPointsLocalMap.cc, over the rows of the
# key-frame store of LocalMapPointsRefresh.cc), driven by scenes (tests/test_gpu_local_map_dropin.py); Frame.h, KeyFrame.h and MapPoint.h are this
# directory's (they add mnTrackReferenceForFrame and the covisibility list), cvmini.h that of tests/mappoints_dropin
LM_DROPIN := orb_slam_amd/cpp/LocalMapPointsLocalMap.cc orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPoints.cc orb_slam_amd/cpp/LocalMapPoints.h \
    orb_slam_amd/cpp/ORBmatcherAccess.h $(wildcard tests/localmap_dropin/*.h) tests/mappoints_dropin/cvmini.h
tests/localmap_dropin/harness: tests/localmap_dropin/harness.cpp $(LM_DROPIN) include/orbp.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/localmap_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/LocalMapPoints.cc \
	    orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPointsLocalMap.cc -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# LocalMapPoints::KeyFrameCulling (orb_slam_amd/cpp/LocalMapPointsCull.cc, over the columns of LocalMapPointsLocalMap.cc and the rows of
# LocalMapPointsRefresh.cc), driven by scenes (tests/test_gpu_cull_dropin.py); Frame.h, KeyFrame.h and MapPoint.h are this directory's (they add
# SetBadFlag, EraseObservation, SetNotErase and the covisibility list), cvmini.h that of tests/mappoints_dropin
CULL_DROPIN := orb_slam_amd/cpp/LocalMapPointsCull.cc orb_slam_amd/cpp/LocalMapPointsLocalMap.cc orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPoints.cc \
    orb_slam_amd/cpp/LocalMapPoints.h orb_slam_amd/cpp/ORBmatcherAccess.h $(wildcard tests/cull_dropin/*.h) tests/mappoints_dropin/cvmini.h
tests/cull_dropin/harness: tests/cull_dropin/harness.cpp $(CULL_DROPIN) include/orbp.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/cull_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/LocalMapPoints.cc \
	    orb_slam_amd/cpp/LocalMapPointsRefresh.cc orb_slam_amd/cpp/LocalMapPointsLocalMap.cc orb_slam_amd/cpp/LocalMapPointsCull.cc -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# the Initializer drop-in (orb_slam_amd/cpp/Initializer.cc over include/orbi.h) over a stand-in Frame.h, driven by scenes (tests/test_gpu_init_dropin.py);
# cvmini.h is that of tests/mappoints_dropin.  harness_host is the same class linked against the host route (tools/libinit_host.so exports the C ABI of
# orbi.h on one host core): tests/test_init_dropin_host.py and tools/bench_init.py
INIT_DROPIN := orb_slam_amd/cpp/Initializer.cc orb_slam_amd/cpp/Initializer.h tests/init_dropin/Frame.h tests/mappoints_dropin/cvmini.h orb_slam_amd/csrc/orb_jacobi.h include/orbi.h
tests/init_dropin/harness: tests/init_dropin/harness.cpp $(INIT_DROPIN) include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -ffp-contract=off -Itests/init_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp -Iorb_slam_amd/csrc $< orb_slam_amd/cpp/Initializer.cc -o $@ \
	    -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib
tests/init_dropin/harness_host: tests/init_dropin/harness.cpp $(INIT_DROPIN) tools/libinit_host.so
	$(CXX) -O2 -std=c++14 -Wall -ffp-contract=off -Itests/init_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp -Iorb_slam_amd/csrc $< orb_slam_amd/cpp/Initializer.cc -o $@ \
	    -Ltools -linit_host -Wl,-rpath,'$$ORIGIN/../../tools'

# the PnPsolver drop-in (orb_slam_amd/cpp/PnPsolver.cc over include/orbe.h) over a stand-in Frame.h, driven by scenes (tests/test_gpu_pnp_dropin.py); MapPoint.h
# and cvmini.h are those of tests/mappoints_dropin.  harness_host is the same class linked against the host route (tools/libpnp_host.so):
# tests/test_pnp_dropin_host.py
PNP_DROPIN := orb_slam_amd/cpp/PnPsolver.cc orb_slam_amd/cpp/PnPsolver.h tests/pnp_dropin/Frame.h tests/mappoints_dropin/MapPoint.h tests/mappoints_dropin/cvmini.h include/orbe.h
tests/pnp_dropin/harness: tests/pnp_dropin/harness.cpp $(PNP_DROPIN) include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/pnp_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/PnPsolver.cc -o $@ \
	    -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib
tests/pnp_dropin/harness_host: tests/pnp_dropin/harness.cpp $(PNP_DROPIN) tools/libpnp_host.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/pnp_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/PnPsolver.cc -o $@ \
	    -Ltools -lpnp_host -Wl,-rpath,'$$ORIGIN/../../tools'

# the NewMapPoints drop-in (orb_slam_amd/cpp/NewMapPoints.cc) over a stand-in KeyFrame.h, driven by scripts
# (tests/test_gpu_triangulate_dropin.py); cvmini.h is that of tests/mappoints_dropin
TRI_DROPIN := orb_slam_amd/cpp/NewMapPoints.cc orb_slam_amd/cpp/NewMapPoints.h tests/triangulate_dropin/KeyFrame.h tests/mappoints_dropin/cvmini.h
tests/triangulate_dropin/harness: tests/triangulate_dropin/harness.cpp $(TRI_DROPIN) include/orbt.h include/orbs.h include/orbf.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -Wall -Itests/triangulate_dropin -Itests/mappoints_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/NewMapPoints.cc -o $@ \
	    -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# the host route tools/bench_triangulate.py measures the device triangulation against (one host core); tests/test_triangulate_host.py
# holds it against the numpy restatement
tools/libtriangulate_host.so: tools/triangulate_host_route.cpp include/orbt.h
	$(CXX) -O2 -std=c++14 -ffp-contract=off -fPIC -shared -Iinclude $< -o $@

# the host route tools/bench_refresh.py measures orbp_refresh against (one host core; -mpopcnt: the reference builds with -march=native)
tools/librefresh_host.so: tools/refresh_host_route.cpp include/orbp.h
	$(CXX) -O2 -std=c++14 -ffp-contract=off -mpopcnt -fPIC -shared -Iinclude $< -o $@

# the host route tools/bench_fuse.py measures orbp_fuse against: the projection of ORBmatcher::Fuse on one host core, in front of the window search
tools/libfuse_host.so: tools/fuse_host_route.cpp include/orbp.h
	$(CXX) -O2 -std=c++14 -ffp-contract=off -fPIC -shared -Iinclude $< -o $@

# the host route tools/bench_loop.py measures orbp_loop_search and orbp_fuse over a similarity against: the decomposition of Scw and the projection on one host core
tools/libloop_host.so: tools/loop_host_route.cpp tools/fuse_host_route.cpp include/orbp.h
	$(CXX) -O2 -std=c++14 -ffp-contract=off -fPIC -shared -Iinclude $< -o $@

# the host route tools/bench_sim3.py measures orbp_sim3_search against: the pair arithmetic and the projection of both directions on one host core, packed as queries
tools/libsim3_host.so: tools/sim3_host_route.cpp include/orbp.h
	$(CXX) -O2 -std=c++14 -ffp-contract=off -fPIC -shared -Iinclude $< -o $@

# the host route tools/bench_init.py measures the monocular initialisation (orbi_models, orbi_check_rt) against: the same algorithm with the same
# double Jacobi iteration on one host core; tests/test_init_host.py holds it against the numpy restatement
tools/libinit_host.so: tools/init_host_route.cpp include/orbi.h orb_slam_amd/csrc/orbi_math.h orb_slam_amd/csrc/orb_jacobi.h
	$(CXX) -O2 -std=c++14 -ffp-contract=off -fPIC -shared -Iinclude -Iorb_slam_amd/csrc $< -o $@

# the host route tools/bench_pnp.py measures the EPnP RANSAC of the relocalisation (orbe_hypotheses, orbe_refine, orbe_select, orbe_iterate) against:
# the C ABI of include/orbe.h on one host core over the same arithmetic text; tests/test_pnp_host.py holds it against the numpy restatement
tools/libpnp_host.so: tools/pnp_host_route.cpp include/orbe.h orb_slam_amd/csrc/orbe_math.h orb_slam_amd/csrc/orbe_host.h orb_slam_amd/csrc/orb_jacobi.h
	$(CXX) -O2 -std=c++14 -Wall -ffp-contract=off -fPIC -shared -Iinclude -Iorb_slam_amd/csrc $< -o $@

# the host route tools/bench_local_map.py measures the local-map chain against: the three object-graph walks over flat stand-in arrays on one host core
tools/liblocalmap_host.so: tools/local_map_host_route.cpp
	$(CXX) -O2 -std=c++14 -fPIC -shared $< -o $@

# the host route tools/bench_cull.py measures orbp_cull against: LocalMapping::KeyFrameCulling over flat stand-in arrays with a std::map per point, one host core
tools/libcull_host.so: tools/cull_host_route.cpp
	$(CXX) -O2 -std=c++14 -fPIC -shared $< -o $@

# the host-query route tools/bench_source_track.py measures the device-resident last-frame / key-frame searches against (one host core)
tools/libsource_host.so: tools/source_host_route.cpp include/orbp.h
	$(CXX) -O2 -std=c++14 -ffp-contract=off -fPIC -shared -Iinclude $< -o $@

# the host-query route tools/bench_mappoints.py measures the device map-point table against (one host core)
tools/libmappoints_host.so: tools/mappoints_host_route.cpp include/orbp.h
	$(CXX) -O2 -std=c++14 -ffp-contract=off -fPIC -shared -Iinclude $< -o $@

# measurement aid: issue rate of the VALU opcodes the kernels are made of (profiles/r01_valu_issue_rates.txt)
tools/microbench/valu_rate: tools/microbench/valu_rate.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-value $< -o $@
tools/microbench/valu_rate2: tools/microbench/valu_rate2.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-value $< -o $@
tools/microbench/mfma_layout: tools/microbench/mfma_layout.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-result $< -o $@
tools/microbench/mfma_layout_fp4: tools/microbench/mfma_layout_fp4.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-value $< -o $@
tools/microbench/mfma_valu_mix: tools/microbench/mfma_valu_mix.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-result $< -o $@
tools/microbench/fetch_calib: tools/microbench/fetch_calib.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-result $< -o $@
# round 4: VALU issue cost against the EXEC mask; vector-memory cost against the access shape (profiles/r04_valu_exec_mask.txt, r04_ta_shapes.txt)
tools/microbench/valu_exec_mask: tools/microbench/valu_exec_mask.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-value $< -o $@
tools/microbench/ta_shapes: tools/microbench/ta_shapes.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++20 -Wno-unused-value $< -o $@

clean:
	rm -f tools/libpnp_host.so tests/pnp_dropin/harness tests/pnp_dropin/harness_host tests/init_dropin/harness tests/init_dropin/harness_host tools/libinit_host.so tools/libcull_host.so tests/cull_dropin/harness tests/localmap_dropin/harness tools/liblocalmap_host.so tests/newpoints_dropin/harness tests/bow_dropin/harness tests/sim3_dropin/harness tools/libsim3_host.so tests/loop_dropin/harness tests/fuse_dropin/harness tools/libfuse_host.so tools/libloop_host.so tests/refresh_dropin/harness tests/mappoints_dropin/harness tests/source_dropin/harness tests/triangulate_dropin/harness tools/libmappoints_host.so tools/libsource_host.so tools/libtriangulate_host.so tools/librefresh_host.so tools/microbench/mfma_layout_fp4 tools/microbench/valu_exec_mask tools/microbench/ta_shapes tools/microbench/valu_rate tools/microbench/valu_rate2 tools/microbench/mfma_layout tools/microbench/mfma_valu_mix tools/microbench/fetch_calib orb_slam_amd/cpp/bench_single_frame tests/kfdb_dropin/harness orb_slam_amd/cpp/example_lanes orb_slam_amd/cpp/example_frame orb_slam_amd/cpp/example_batch orb_slam_amd/cpp/example_color orb_slam_amd/cpp/example_pipeline orb_slam_amd/liborbx.so orb_slam_amd/libsynthframes.so oracle/liborb_oracle.so
	rm -rf oracle/_ref oracle/_ref_native build/orbx

.PHONY: all clean oracle_ref
