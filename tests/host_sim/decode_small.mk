# tests/host_sim/decode_small.mk: the decoder role at the ring of decode_small_kernel (nlzm_amd/csrc/nlzm_decode_small.hip), run on the CPU,
# every lane a fiber (xw_sim.cpp), beside the host decoder.  TEST HARNESS ONLY (tests/test_decode_small_ring_sim.py).  Under UBSan, as the
# mutant runs of decode.mk are (AddressSanitizer does not follow the fibers' hand-switched stacks: PROT_NONE pages and canaries instead).
RING ?= 16384
SRC  = decode_small_sim.cpp xw_sim.cpp
DEPS = $(SRC) decode_sim.cpp ../../nlzm_amd/csrc/nlzm_decode.h ../../nlzm_amd/csrc/nlzm_host_decode.h ../../nlzm_amd/csrc/xw.h
CXXFLAGS = -O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function
all: decode_small_sim
decode_small_sim: $(DEPS)
	g++ $(CXXFLAGS) -DNLZM_DEC_RING=$(RING) -fsanitize=undefined -fno-sanitize-recover=undefined -o $@ $(SRC)
clean:
	rm -f decode_small_sim
