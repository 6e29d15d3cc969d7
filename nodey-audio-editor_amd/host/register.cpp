// register.cpp — fills Processor::processor_map with the GPU processors, under the identifiers of the CPU classes
// they replace (reference list: src/register.cpp:16-23).  audio_input / audio_output are codec and device I/O and
// stay the reference's own classes; audio_spectrum is new.  Nodes the reference has no class for (audio_filter) are registered by a call of
// their own, register_extension_processors(), so that register_all_processors() stays the mirror of the reference's list.
#include "infra/processor.hpp"
#include "processor/audio-filter.hpp"
#include "processor/audio-reverb.hpp"
#include "processor/audio-eq.hpp"
#include "processor/audio-dynamics.hpp"
#include "processor/audio-denoise.hpp"
#include "processor/audio-loudness.hpp"
#include "processor/audio-sidechain.hpp"
#include "processor/audio-echo.hpp"
#include "processor/audio-modulation.hpp"
#include "processor/audio-saturation.hpp"
#include "processor/audio-gate.hpp"
#include "processor/audio-multiband.hpp"
#include "processor/audio-separation.hpp"
#include "processor/audio-limiter.hpp"
#include "processor/audio-dither.hpp"
#include "processor/audio-mix.hpp"
#include "processor/audio-velocity.hpp"
#include "processor/audio-vol.hpp"

namespace infra
{
	namespace
	{
		template <typename... Nodes>
		void register_each()
		{
			(Processor::register_processor<Nodes>(), ...);
		}
	}

	void register_all_processors(processor::Stretch_algorithm default_algorithm)
	{
		using namespace processor;
		set_default_stretch_algorithm(default_algorithm);
		register_each<Audio_vol, Velocity_modifier, Pitch_modifier, Audio_amix, Audio_bimix, Audio_bimix_v2, Audio_spectrum>();
	}

	// the reference's signature (src/register.cpp:14, called from App::App): the vocoder is this library's default
	void register_all_processors() { register_all_processors(processor::Stretch_algorithm::Vocoder); }

	// the nodes beyond the reference's list; the editor calls it after register_all_processors()
	void register_extension_processors() { register_each<processor::Audio_filter>(); }

	// the effects built on the long convolution; a call of its own, so register_extension_processors() stays the list it was
	void register_effect_processors() { register_each<processor::Audio_reverb>(); }

	// the equalizer on the biquad cascade; again a call of its own, so the three lists above stay what they were
	void register_equalizer_processors() { register_each<processor::Audio_eq>(); }

	// the compressor / limiter on the dynamics processor; a call of its own once more, so the four lists above stay what they were
	void register_dynamics_processors() { register_each<processor::Audio_dynamics>(); }

	// the restoration tools: noise reduction on the spectral gate; a call of its own, so the five lists above stay what they were
	void register_restoration_processors() { register_each<processor::Audio_denoise>(); }

	// the mastering tools: loudness normalization on the BS.1770 meter; a call of its own, so the six lists above stay what they were
	void register_mastering_processors() { register_each<processor::Audio_loudness>(); }

	// the side-chain compressor on the keyed dynamics; a call of its own, so the seven lists above stay what they were
	void register_sidechain_processors() { register_each<processor::Audio_sidechain>(); }

	// the delay effects: the echo; a call of its own, so the eight lists above stay what they were
	void register_echo_processors() { register_each<processor::Audio_echo>(); }

	// the modulation effects: chorus, flanger and vibrato on the modulated delay; a call of its own, so the nine lists above stay what they were
	void register_modulation_processors() { register_each<processor::Audio_modulation>(); }

	// the nonlinear effects: drive, saturation and clipping; a call of its own, so the ten lists above stay what they were
	void register_saturation_processors() { register_each<processor::Audio_saturation>(); }

	// the gate and downward expander; a call of its own, so the eleven lists above stay what they were
	void register_gate_processors() { register_each<processor::Audio_gate>(); }

	// the multiband compressor; a call of its own, so the twelve lists above stay what they were
	void register_multiband_processors() { register_each<processor::Audio_multiband>(); }

	// the harmonic/percussive separation; a call of its own, so the thirteen lists above stay what they were
	void register_separation_processors() { register_each<processor::Audio_separation>(); }

	// the true-peak limiter; a call of its own, so the fourteen lists above stay what they were
	void register_limiter_processors() { register_each<processor::Audio_limiter>(); }

	// the dither; a call of its own, so the fifteen lists above stay what they were
	void register_dither_processors() { register_each<processor::Audio_dither>(); }
}
