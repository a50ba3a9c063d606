# tests/host_sim/decode_steps.mk: the stepping form of the decoder role (dec::decode_role_steps, nlzm_amd/csrc/nlzm_decode.h) run on the CPU,
# every lane a fiber (xw_sim.cpp), beside the one-shot role and the host decoder.  TEST HARNESS ONLY.  decode_steps_sim: the product's ring;
# decode_steps_sim_tiny: the smallest ring the role allows (every resume reloads a ring that most matches reach beyond);
# decode_steps_sim_san: the damaged streams' build, under UBSan (AddressSanitizer does not follow the fibers' hand-switched stacks: the
# harness puts PROT_NONE pages and canaries round every buffer instead, the state record included).
SRC  = decode_steps_sim.cpp xw_sim.cpp
DEPS = $(SRC) ../../nlzm_amd/csrc/nlzm_decode.h ../../nlzm_amd/csrc/nlzm_host_decode.h ../../nlzm_amd/csrc/xw.h
CXXFLAGS = -O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function
all: decode_steps_sim decode_steps_sim_tiny decode_steps_sim_san
decode_steps_sim: $(DEPS)
	g++ $(CXXFLAGS) -o $@ $(SRC)
decode_steps_sim_tiny: $(DEPS)
	g++ $(CXXFLAGS) -DNLZM_DEC_RING=512 -o $@ $(SRC)
decode_steps_sim_san: $(DEPS)
	g++ $(CXXFLAGS) -fsanitize=undefined -fno-sanitize-recover=undefined -o $@ $(SRC)
clean:
	rm -f decode_steps_sim decode_steps_sim_tiny decode_steps_sim_san
