// processor/audio-sidechain.hpp — a node the reference has no class for: a compressor / limiter whose detector listens to a key, on the
// library's keyed dynamics (nae_dynkey_*; DESIGN.md §3, "K15 keyed dynamics").  Registered by infra::register_sidechain_processors().  Its
// process_payload stands in audio-effects.cpp, next to the dynamics node's.
#pragma once
#include "audio-dynamics.hpp"
#include "audio-eq.hpp"

namespace processor
{
	// Registered as "audio_sidechain": two audio input pins, "input" (the signal) and "key" (what the detector listens to), one audio output
	// pin.  An unconnected "key" means the signal is its own key.  JSON keys, all optional: audio_dynamics' nine with their ranges and defaults
	// (audio-dynamics.hpp), and
	//   "key_filter"   an array of 0 ... 4 band objects in audio_eq's format (audio-eq.hpp): the detector hears the key through them
	// "key_filter" of another type, with more than 4 entries or with an entry that is no object: Runtime_error "Wrong field: key_filter"; any
	// other value of the wrong type or outside its range: "Wrong field: <key>".  Defaults are not written back.
	// The key is lined up once, from the first frames of both pins: o = llround((t_key - t_input) rate) with t = pts time_base; the key sample
	// for input sample n is key[n - o], and zero outside what the key stream delivered.  The key stream is one continuous signal from its first
	// frame.  An input sample is put when its key sample has arrived or the key stream has ended; frames of both pins are taken at once into
	// the node's own lists, so a full queue on one pin cannot stall the other.  On the first frames a key of another sample rate, a key with
	// more channels than 1 or the input's, a look-ahead of more than 1024 samples at the stream's rate and a filter band at or above Nyquist
	// are Runtime_errors.  The node delivers exactly the input's frames, as packed float frames of their sizes, pts and time base.
	class Audio_sidechain : public infra::Processor
	{
	  public:

		static constexpr size_t max_bands = 4;   // NAE_DYNKEY_MAX_SECTIONS
		Dynamics_settings dynamics;
		std::vector<Audio_eq::Band> key_filter;

		static infra::Processor::Info get_processor_info();
		Processor::Info get_processor_info_non_static() const override { return get_processor_info(); }
		void draw_title() override;                         // bodies: draw-headless.cpp
		bool draw_content(bool readonly) override;
		std::vector<infra::Processor::Pin_attribute> get_pin_attributes() const override;
		void process_payload(
			const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
			const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
			const std::atomic<bool>& stop_token,
			std::any& user_data
		) override;
		Json::Value serialize() const override;
		void deserialize(const Json::Value& value) override;
	};
}
