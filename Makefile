# Build the MI355X POST engine (libpost_hip.so, gfx950) and the CPU oracle.
# hipcc cross-compiles gfx950 without a GPU; the in-tree .so travels to the
# GPU box with the gpurun snapshot.
HIPCC   ?= hipcc
ARCH    ?= gfx950
HIPFLAGS ?= --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall

ENGINE  := go-spacemesh_amd/libpost_hip.so
CSRC    := go-spacemesh_amd/csrc

all: $(ENGINE) oracle

SRCS_ENGINE := $(CSRC)/kernels.hip $(CSRC)/engine.cpp $(CSRC)/crypto_host.cpp
HDRS_ENGINE := $(CSRC)/post_common.h $(CSRC)/kernel_args.h \
               $(CSRC)/crypto_host.h $(CSRC)/hip_owned.h \
               $(CSRC)/init_proof_host.h include/spacemesh_post.h

$(ENGINE): $(SRCS_ENGINE) $(HDRS_ENGINE)
	$(HIPCC) $(HIPFLAGS) -shared $(SRCS_ENGINE) -o $@

# A/B variant: non-temporal scratch access (POST_ENGINE_LIB selects)
go-spacemesh_amd/libpost_hip_nt.so: $(SRCS_ENGINE) $(HDRS_ENGINE)
	$(HIPCC) $(HIPFLAGS) -DPOSTE_NT=1 -shared $(SRCS_ENGINE) -o $@

nt: go-spacemesh_amd/libpost_hip_nt.so
.PHONY: nt

# A/B variant: scan ILP depth 4
go-spacemesh_amd/libpost_hip_scan4.so: $(SRCS_ENGINE) $(HDRS_ENGINE)
	$(HIPCC) $(HIPFLAGS) -DPOSTE_SCAN_ILP=4 -shared $(SRCS_ENGINE) -o $@
scan4: go-spacemesh_amd/libpost_hip_scan4.so
.PHONY: scan4

# A/B variant: scan ILP depth 1
go-spacemesh_amd/libpost_hip_scan1.so: $(SRCS_ENGINE) $(HDRS_ENGINE)
	$(HIPCC) $(HIPFLAGS) -DPOSTE_SCAN_ILP=1 -shared $(SRCS_ENGINE) -o $@
scan1: go-spacemesh_amd/libpost_hip_scan1.so
.PHONY: scan1

# Host check of the owning handles (csrc/hip_owned.h) under ASan + UBSan: a
# stand-alone program, needs no GPU (without one every creating call fails,
# which is the path that must not double-free).  Not part of `all`.
tools/hip_owned_test: tools/hip_owned_test.cpp $(CSRC)/hip_owned.h
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -Wall \
	    -Xarch_host -fsanitize=address,undefined $< -o $@
hip_owned_test: tools/hip_owned_test
	./tools/hip_owned_test
.PHONY: hip_owned_test

# Host check of the initial proof's part files (csrc/init_proof_host.h: parse,
# truncate, merge, tiling, winner) under ASan + UBSan: a stand-alone program,
# no GPU and no HIP.  DIR holds postdata_hits.part-* files, TOTAL is the dir's
# label count.  Not part of `all`.
tools/init_proof_host_test: tools/init_proof_host_test.cpp \
    $(CSRC)/init_proof_host.h $(CSRC)/crypto_host.cpp $(CSRC)/crypto_host.h
	$(CXX) -O1 -g -std=c++17 -Wall -pthread -fsanitize=address,undefined \
	    -fno-sanitize-recover=undefined tools/init_proof_host_test.cpp \
	    $(CSRC)/crypto_host.cpp -o $@
init_proof_host_test: tools/init_proof_host_test
	./tools/init_proof_host_test $(DIR) $(TOTAL)
.PHONY: init_proof_host_test

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(ENGINE) tools/hip_owned_test tools/init_proof_host_test
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
