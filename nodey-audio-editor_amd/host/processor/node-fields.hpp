// processor/node-fields.hpp — a node's parameters stated once.  The parameters are a plain copyable record the node derives from (Gate_settings,
// Dynamics_settings, ...); next to it, in audio-effects.cpp, stands ONE list of fields: std::tuple{Number{...}, Choice{...}, Flag{...}, ...} in the
// order the keys are read.  A field names its JSON key, its member, the default and the bounds, and from the list
//   to_json    writes what differs from the defaults,
//   from_json  reads and checks every key, in the list's order, into a fresh record -> the record; the first wrong key throws "Wrong field: <key>"
//              (wrong_field), so the caller assigns only what passed as a whole,
//   clamp      keeps every number inside its bounds: what the widgets would keep (draw-headless.cpp).
// What a plain closed range does not say is a Rule at the field: `ok` is checked behind the range, at the field's place in the order, and only
// for a key that is there; `keep` stands in for std::clamp(v, lo, hi).  A node may put a field type of its own into its list (the reverb's
// seed): anything with write, read and keep.
#pragma once
#include "node-util.hpp"

#include <algorithm>
#include <optional>
#include <tuple>
#include <type_traits>

namespace processor::detail
{
	// a number arrives as JSON's double or, for an integer member, as int (real_from_json, int_from_json): `ok` sees it before a float member narrows it
	template <class T> using Json_number = std::conditional_t<std::is_integral_v<T>, int, double>;

	template <class T>
	struct Rule
	{
		bool (*ok)(Json_number<T> v, Json_number<T> lo, Json_number<T> hi) = nullptr;
		T (*keep)(T v, T lo, T hi) = nullptr;
	};

	// the rules more than one node has.  The range's lower bound is open: 0 itself is no value; clamp starts at Floor
	template <auto Floor>
	inline constexpr Rule<decltype(Floor)> above_lo{
		[](double v, double lo, double) { return v > lo; }, [](decltype(Floor) v, decltype(Floor), decltype(Floor) hi) { return std::clamp(v, Floor, hi); }};
	// ... and clamp has no ceiling
	template <auto Floor>
	inline constexpr Rule<decltype(Floor)> above_lo_unbounded{
		[](double v, double lo, double) { return v > lo; }, [](decltype(Floor) v, decltype(Floor), decltype(Floor)) { return std::max(v, Floor); }};
	// a corner frequency: lo (0) for none, else From ... hi; clamp leaves 0 alone
	template <auto From>
	inline constexpr Rule<decltype(From)> none_or_from{
		[](double v, double lo, double) { return v == lo || v >= From; },
		[](decltype(From) v, decltype(From) lo, decltype(From) hi) { return v == lo ? v : std::clamp(v, From, hi); }};
	// read and checked, but not clamped (a frame size, 0 for the library's pick)
	template <class T> T as_it_is(T v, T, T) { return v; }

	// a real (double or float member) or an integer in [lo, hi]
	template <class Rec, class T>
	struct Number
	{
		const char* key;
		T Rec::*member;
		T fallback;
		Json_number<T> lo, hi;
		Rule<T> rule = {};

		Json_number<T> checked(const Json::Value& value, const char* node_name) const
		{
			Json_number<T> v;
			if constexpr (std::is_integral_v<T>) v = int_from_json(value, node_name, key, lo, hi, fallback);
			else v = real_from_json(value, node_name, key, lo, hi, fallback);
			if (rule.ok && value.isMember(key) && !rule.ok(v, lo, hi)) throw wrong_field(node_name, key);
			return v;
		}
		T kept(T v) const { return rule.keep ? rule.keep(v, (T)lo, (T)hi) : std::clamp(v, (T)lo, (T)hi); }

		void write(const Rec& r, Json::Value& value) const { if (r.*member != fallback) value[key] = r.*member; }
		void read(Rec& r, const Json::Value& value, const char* node_name) const { r.*member = (T)checked(value, node_name); }
		void keep(Rec& r) const { r.*member = kept(r.*member); }
	};

	// a real that may be absent: no key is no value, and no value is not written
	template <class Rec>
	struct Optional_real
	{
		const char* key;
		std::optional<double> Rec::*member;
		double lo, hi;
		Rule<double> rule = {};

		Number<Rec, double> number() const { return {key, nullptr, 0.0, lo, hi, rule}; }
		void write(const Rec& r, Json::Value& value) const { if ((r.*member).has_value()) value[key] = *(r.*member); }
		void read(Rec& r, const Json::Value& value, const char* node_name) const
		{
			r.*member = value.isMember(key) ? std::optional<double>(number().checked(value, node_name)) : std::nullopt;
		}
		void keep(Rec& r) const { if ((r.*member).has_value()) r.*member = number().kept(*(r.*member)); }
	};

	// a bool, written only when it is not the default; not clamped
	template <class Rec>
	struct Flag
	{
		const char* key;
		bool Rec::*member;
		bool fallback;

		void write(const Rec& r, Json::Value& value) const { if (r.*member != fallback) value[key] = r.*member; }
		void read(Rec& r, const Json::Value& value, const char* node_name) const { r.*member = bool_from_json(value, node_name, key, fallback); }
		void keep(Rec&) const {}
	};

	// an enum by its names, in the enumerators' order from 0: the first is the default and is not written; not clamped
	template <class Rec, class E, size_t N>
	struct Choice
	{
		const char* key;
		E Rec::*member;
		const char* const (&names)[N];

		void write(const Rec& r, Json::Value& value) const { if (r.*member != E(0)) value[key] = names[(size_t)(r.*member)]; }
		void read(Rec& r, const Json::Value& value, const char* node_name) const
		{
			r.*member = E(0);
			if (!value.isMember(key)) return;
			size_t found = 0;
			while (found < N && !(value[key].isString() && value[key].asString() == names[found])) found++;
			if (found == N) throw wrong_field(node_name, key);
			r.*member = E(found);
		}
		void keep(Rec&) const {}
	};

	template <class Rec, class... Fields>
	Json::Value to_json(const Rec& record, const std::tuple<Fields...>& fields)
	{
		Json::Value value;
		std::apply([&](const auto&... f) { (f.write(record, value), ...); }, fields);
		return value;
	}

	template <class Rec, class... Fields>
	Rec from_json(const Json::Value& value, const char* node_name, const std::tuple<Fields...>& fields)
	{
		Rec record;
		std::apply([&](const auto&... f) { (f.read(record, value, node_name), ...); }, fields);
		return record;
	}

	template <class Rec, class... Fields>
	void clamp(Rec& record, const std::tuple<Fields...>& fields)
	{
		std::apply([&](const auto&... f) { (f.keep(record), ...); }, fields);
	}
}
