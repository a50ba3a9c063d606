# tests/host_sim/decode.mk: the decoder role (nlzm_amd/csrc/nlzm_decode.h) run on the CPU, every lane a fiber (xw_sim.cpp), beside the
# host decoder.  TEST HARNESS ONLY.  decode_sim: the product's ring; decode_sim_tiny: the smallest ring the role allows (nearly every
# match comes from "memory", copies straddle flushes constantly); decode_sim_san: the mutant runs' build, under UBSan
# (AddressSanitizer does not follow the fibers' hand-switched stacks: the harness puts PROT_NONE pages and canaries round every buffer
# instead).
SRC  = decode_sim.cpp xw_sim.cpp
DEPS = $(SRC) ../../nlzm_amd/csrc/nlzm_decode.h ../../nlzm_amd/csrc/nlzm_host_decode.h ../../nlzm_amd/csrc/xw.h
CXXFLAGS = -O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function
all: decode_sim decode_sim_tiny decode_sim_san
decode_sim: $(DEPS)
	g++ $(CXXFLAGS) -o $@ $(SRC)
decode_sim_tiny: $(DEPS)
	g++ $(CXXFLAGS) -DNLZM_DEC_RING=512 -o $@ $(SRC)
decode_sim_san: $(DEPS)
	g++ $(CXXFLAGS) -fsanitize=undefined -fno-sanitize-recover=undefined -o $@ $(SRC)
clean:
	rm -f decode_sim decode_sim_tiny decode_sim_san
