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

# what `all` builds and `clean` removes, named once
LIBS             := orb_slam_amd/liborbx.so orb_slam_amd/libsynthframes.so oracle/liborb_oracle.so
EXAMPLES         := $(addprefix orb_slam_amd/cpp/,example_frame example_batch example_color example_pipeline example_lanes bench_single_frame)
DROPIN_HARNESSES := $(patsubst %,tests/%_dropin/harness,kfdb mappoints source triangulate refresh fuse loop sim3 bow newpoints localmap cull init pnp sim3solver poseopt) \
    tests/init_dropin/harness_host tests/pnp_dropin/harness_host tests/sim3solver_dropin/harness_host tests/poseopt_dropin/harness_host \
    tests/localba_dropin/harness tests/localba_dropin/harness_host tests/sim3opt_dropin/harness tests/sim3opt_dropin/harness_host
HOST_ROUTE_LIBS  := $(patsubst %,tools/lib%_host.so,mappoints localmap cull source triangulate refresh fuse loop sim3 init pnp sim3solver poseopt localba sim3opt)
MICROBENCH       := $(addprefix tools/microbench/,valu_rate valu_rate2 mfma_layout mfma_layout_fp4 mfma_valu_mix fetch_calib valu_exec_mask ta_shapes)

all: $(LIBS) oracle_ref $(EXAMPLES) $(DROPIN_HARNESSES) build/dropin/tracking_only.ok $(HOST_ROUTE_LIBS) $(MICROBENCH)

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

# the KeyFrameDatabase drop-in (orb_slam_amd/cpp/KeyFrameDatabase.cc) over its own stand-in KeyFrame.h / Frame.h (they sit on cvcompat.h), driven by
# scripts (tests/test_gpu_kfdb_dropin.py)
KFDB_DROPIN := orb_slam_amd/cpp/KeyFrameDatabase.cc orb_slam_amd/cpp/KeyFrameDatabase.h orb_slam_amd/cpp/ORBVocabulary.h tests/kfdb_dropin/KeyFrame.h tests/kfdb_dropin/Frame.h
tests/kfdb_dropin/harness: tests/kfdb_dropin/harness.cpp $(KFDB_DROPIN) include/orbd.h include/orbv.h include/orbx.h orb_slam_amd/liborbx.so
	$(CXX) -O2 -std=c++14 -pthread -Itests/kfdb_dropin -Iinclude -Iorb_slam_amd/cpp $< orb_slam_amd/cpp/KeyFrameDatabase.cc -o $@ -Lorb_slam_amd -lorbx \
	    -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib

# the BundleAdjuster drop-in (orb_slam_amd/cpp/BundleAdjuster.cc) over its own stand-in KeyFrame.h / MapPoint.h / Map.h (tests/standin lacks SetPose, GetInvSigma2,
# the mnBA* marks and EraseObservation's bad rule; they sit on its cvmini.h), driven by scenes (tests/test_gpu_localba_dropin.py); harness_host is the same
# class linked against the host route (tests/test_localba_dropin_host.py)
LOCALBA_DROPIN := orb_slam_amd/cpp/BundleAdjuster.cc orb_slam_amd/cpp/BundleAdjuster.h $(addprefix tests/localba_dropin/,KeyFrame.h MapPoint.h Map.h) tests/standin/cvmini.h \
    include/orbb.h include/orbo.h include/orbx.h
LOCALBA_CXXFLAGS := -O2 -std=c++14 -Wall -Itests/localba_dropin -Itests/standin -Iinclude -Iorb_slam_amd/cpp
tests/localba_dropin/harness: tests/localba_dropin/harness.cpp $(LOCALBA_DROPIN) orb_slam_amd/liborbx.so
	$(CXX) $(LOCALBA_CXXFLAGS) $< orb_slam_amd/cpp/BundleAdjuster.cc -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib
tests/localba_dropin/harness_host: tests/localba_dropin/harness.cpp $(LOCALBA_DROPIN) tools/liblocalba_host.so
	$(CXX) $(LOCALBA_CXXFLAGS) $< orb_slam_amd/cpp/BundleAdjuster.cc -o $@ -Ltools -llocalba_host -Wl,-rpath,'$$ORIGIN/../../tools'

# the Sim3Optimizer drop-in (orb_slam_amd/cpp/Sim3Optimizer.cc) over its own stand-in KeyFrame.h / MapPoint.h / Sim3.h (tests/standin lacks GetInvSigma2 and
# GetCalibrationMatrix; Sim3.h has g2o's accessor names, so the template overload runs), driven by scenes (tests/test_gpu_sim3opt_dropin.py); harness_host is
# the same class linked against the host route (tests/test_sim3opt_dropin_host.py).  Sim3Optimizer.cc shares orbg_math.h with the kernel and rounds as it does.
SIM3OPT_DROPIN := orb_slam_amd/cpp/Sim3Optimizer.cc orb_slam_amd/cpp/Sim3Optimizer.h $(addprefix tests/sim3opt_dropin/,KeyFrame.h MapPoint.h Sim3.h) tests/standin/cvmini.h \
    include/orbg.h include/orbo.h include/orbx.h orb_slam_amd/csrc/orbg_math.h orb_slam_amd/csrc/orbo_math.h orb_slam_amd/csrc/orb_jacobi.h
SIM3OPT_CXXFLAGS := -O2 -std=c++14 -Wall -ffp-contract=off -Itests/sim3opt_dropin -Itests/standin -Iinclude -Iorb_slam_amd/cpp -Iorb_slam_amd/csrc
tests/sim3opt_dropin/harness: tests/sim3opt_dropin/harness.cpp $(SIM3OPT_DROPIN) orb_slam_amd/liborbx.so
	$(CXX) $(SIM3OPT_CXXFLAGS) $< orb_slam_amd/cpp/Sim3Optimizer.cc -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib
tests/sim3opt_dropin/harness_host: tests/sim3opt_dropin/harness.cpp $(SIM3OPT_DROPIN) tools/libsim3opt_host.so
	$(CXX) $(SIM3OPT_CXXFLAGS) $< orb_slam_amd/cpp/Sim3Optimizer.cc -o $@ -Ltools -lsim3opt_host -Wl,-rpath,'$$ORIGIN/../../tools'

# The other drop-in classes (orb_slam_amd/cpp/LocalMapPoints*.cc, NewMapPoints.cc, Initializer.cc, PnPsolver.cc, Sim3Solver.cc, PoseOptimizer.cc) are compiled once, against the one set
# of stand-in ORB_SLAM classes in tests/standin, into one archive.  tests/NAME_dropin/harness.cpp drives them through scripts or scenes
# (tests/test_gpu_NAME_dropin.py); the linker takes the members a harness needs.  harness_host is the same harness and class linked against the host
# route of the C ABI (tools/libNAME_host.so) in liborbx's place: tests/test_init_dropin_host.py, tests/test_pnp_dropin_host.py, tests/test_sim3solver_dropin_host.py, tests/test_poseopt_dropin_host.py, tools/bench_init.py.
DROPIN_CXXFLAGS := -O2 -std=c++14 -Wall -Itests/standin -Iinclude -Iorb_slam_amd/cpp
DROPIN_HDRS := $(wildcard tests/standin/*.h orb_slam_amd/cpp/*.h include/*.h)
DROPIN_OBJS := $(patsubst orb_slam_amd/cpp/%.cc,build/dropin/%.o,$(wildcard orb_slam_amd/cpp/LocalMapPoints*.cc) $(addprefix orb_slam_amd/cpp/,NewMapPoints.cc Initializer.cc PnPsolver.cc Sim3Solver.cc PoseOptimizer.cc))
DROPIN_LIB  := build/dropin/libdropin.a
# Initializer.cc shares orb_jacobi.h with the kernels and must round as they do (private: what these targets cause to be built does not inherit it)
build/dropin/Initializer.o tests/init_dropin/harness tests/init_dropin/harness_host: private DROPIN_CXXFLAGS += -ffp-contract=off -Iorb_slam_amd/csrc
# Sim3Solver.cc holds the float text of the constructor (Rcw*X+tcw, FromCameraToImage), pinned operation by operation
build/dropin/Sim3Solver.o: private DROPIN_CXXFLAGS += -ffp-contract=off
build/dropin/Initializer.o: orb_slam_amd/csrc/orb_jacobi.h
build/dropin/%.o: orb_slam_amd/cpp/%.cc $(DROPIN_HDRS)
	@mkdir -p build/dropin
	$(CXX) $(DROPIN_CXXFLAGS) -c $< -o $@
$(DROPIN_LIB): $(DROPIN_OBJS)
	rm -f $@ && ar rcs $@ $^
tests/%_dropin/harness: tests/%_dropin/harness.cpp $(DROPIN_LIB) $(DROPIN_HDRS) orb_slam_amd/liborbx.so
	$(CXX) $(DROPIN_CXXFLAGS) $< $(DROPIN_LIB) -o $@ -Lorb_slam_amd -lorbx -Wl,-rpath,'$$ORIGIN/../../orb_slam_amd' -Wl,-rpath,/opt/rocm/lib
tests/init_dropin/harness_host: tests/init_dropin/harness.cpp $(DROPIN_LIB) $(DROPIN_HDRS) tools/libinit_host.so
	$(CXX) $(DROPIN_CXXFLAGS) $< $(DROPIN_LIB) -o $@ -Ltools -linit_host -Wl,-rpath,'$$ORIGIN/../../tools'
tests/pnp_dropin/harness_host: tests/pnp_dropin/harness.cpp $(DROPIN_LIB) $(DROPIN_HDRS) tools/libpnp_host.so
	$(CXX) $(DROPIN_CXXFLAGS) $< $(DROPIN_LIB) -o $@ -Ltools -lpnp_host -Wl,-rpath,'$$ORIGIN/../../tools'
tests/sim3solver_dropin/harness_host: tests/sim3solver_dropin/harness.cpp $(DROPIN_LIB) $(DROPIN_HDRS) tools/libsim3solver_host.so
	$(CXX) $(DROPIN_CXXFLAGS) $< $(DROPIN_LIB) -o $@ -Ltools -lsim3solver_host -Wl,-rpath,'$$ORIGIN/../../tools'
tests/poseopt_dropin/harness_host: tests/poseopt_dropin/harness.cpp $(DROPIN_LIB) $(DROPIN_HDRS) tools/libposeopt_host.so
	$(CXX) $(DROPIN_CXXFLAGS) $< $(DROPIN_LIB) -o $@ -Ltools -lposeopt_host -Wl,-rpath,'$$ORIGIN/../../tools'
# LocalMapPoints.cc and LocalMapPointsSource.cc promise to name nothing of MapPoint and KeyFrame beyond what the tracking searches need: they compile
# against the stand-ins with everything else taken away
build/dropin/tracking_only.ok: orb_slam_amd/cpp/LocalMapPoints.cc orb_slam_amd/cpp/LocalMapPointsSource.cc $(DROPIN_HDRS)
	@mkdir -p build/dropin
	$(CXX) $(DROPIN_CXXFLAGS) -DSTANDIN_TRACKING_ONLY -fsyntax-only orb_slam_amd/cpp/LocalMapPoints.cc
	$(CXX) $(DROPIN_CXXFLAGS) -DSTANDIN_TRACKING_ONLY -fsyntax-only orb_slam_amd/cpp/LocalMapPointsSource.cc
	@touch $@

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

# the host route tools/bench_sim3solver.py measures the Sim3 RANSAC of loop closing (orbh_hypotheses, orbh_select, orbh_iterate) against: the C ABI of
# include/orbh.h on one host core over the same arithmetic text; tests/test_sim3solver_host.py holds it against the numpy restatement
tools/libsim3solver_host.so: tools/sim3solver_host_route.cpp include/orbh.h orb_slam_amd/csrc/orbh_math.h orb_slam_amd/csrc/orbh_host.h orb_slam_amd/csrc/orb_jacobi.h
	$(CXX) -O2 -std=c++14 -Wall -ffp-contract=off -fPIC -shared -Iinclude -Iorb_slam_amd/csrc $< -o $@

# the host route tools/bench_poseopt.py measures the pose optimisation of tracking (orbo_pose, orbo_pose_batch) against: the host forms of
# include/orbo.h on one host core over the same arithmetic text and summation order; tests/test_poseopt_host.py holds it against the numpy restatement
tools/libposeopt_host.so: tools/poseopt_host_route.cpp include/orbo.h orb_slam_amd/csrc/orbo_math.h orb_slam_amd/csrc/orbo_host.h orb_slam_amd/csrc/orb_jacobi.h
	$(CXX) -O2 -std=c++14 -Wall -ffp-contract=off -fPIC -shared -Iinclude -Iorb_slam_amd/csrc $< -o $@

# the host route tools/bench_localba.py measures the bundle adjustment of the mapping thread (orbb_optimize) against: the host forms of
# include/orbb.h on one host core over the same arithmetic text and summation orders; tests/test_localba_host.py holds it against the numpy restatement
tools/liblocalba_host.so: tools/localba_host_route.cpp include/orbb.h include/orbo.h orb_slam_amd/csrc/orbb_math.h orb_slam_amd/csrc/orbb_host.h orb_slam_amd/csrc/orbo_math.h orb_slam_amd/csrc/orbo_host.h orb_slam_amd/csrc/orb_jacobi.h
	$(CXX) -O2 -std=c++14 -Wall -ffp-contract=off -fPIC -shared -Iinclude -Iorb_slam_amd/csrc $< -o $@

# the host route tools/bench_sim3opt.py measures the Sim3 refinement of loop closing (orbg_sim3, orbg_sim3_batch) against: the host forms of
# include/orbg.h on one host core over the same arithmetic text and summation order; tests/test_sim3opt_host.py holds it against the numpy restatement
tools/libsim3opt_host.so: tools/sim3opt_host_route.cpp include/orbg.h include/orbo.h orb_slam_amd/csrc/orbg_math.h orb_slam_amd/csrc/orbg_host.h orb_slam_amd/csrc/orbo_math.h orb_slam_amd/csrc/orbo_host.h orb_slam_amd/csrc/orb_jacobi.h
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
	rm -f $(LIBS) $(EXAMPLES) $(DROPIN_HARNESSES) $(HOST_ROUTE_LIBS) $(MICROBENCH)
	rm -rf oracle/_ref oracle/_ref_native build/orbx build/dropin

.PHONY: all clean oracle_ref
